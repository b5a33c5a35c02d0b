"""ldp_get_dosage_sums at the three places a caller meets it: the library's exports, the boundary header, the Python binding.  No GPU."""
import ctypes
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_call(pkg):
    L = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "ldp_get_dosage_sums")


def test_the_header_declares_the_call():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ldprune_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+ldp_get_dosage_sums\s*\(([^)]*)\)\s*;", text)
    assert decl, "include/ldprune_hip.h does not declare ldp_get_dosage_sums"
    params = [re.sub(r"\s+", " ", p.strip()) for p in decl.group(1).split(",")]
    assert params == ["ldp_engine* e", "uint32_t first_variant", "uint32_t n", "uint64_t* ref_dosage", "uint64_t* alt_dosage", "uint8_t* has_sums"], params


def test_the_binding_carries_the_call(pkg):
    assert "ldp_get_dosage_sums" in pkg.CABI_SYMBOLS
    fn = pkg.lib().ldp_get_dosage_sums
    assert fn.argtypes is not None and len(fn.argtypes) == 6
    sig = inspect.signature(pkg.LdPruneEngine.dosage_sums)
    assert list(sig.parameters) == ["self", "first", "n"] and sig.parameters["first"].default == 0 and sig.parameters["n"].default is None


def test_null_engine_and_unplanned_engine_are_refused(pkg):
    L = pkg.lib()
    ref, alt, has = (ctypes.c_uint64 * 1)(), (ctypes.c_uint64 * 1)(), (ctypes.c_uint8 * 1)()
    assert L.ldp_get_dosage_sums(None, 0, 1, ref, alt, has) == pkg.LDP_ERR_INVALID
    eng = pkg.LdPruneEngine(64, 10, 1, False, 0.5, device=0)
    assert L.ldp_get_dosage_sums(eng._h, 0, 1, ref, alt, has) == pkg.LDP_ERR_STATE
    # planning is host work: a planned engine answers without a device -- nothing is loaded, so nothing has sums
    import numpy as np
    eng.set_variants(np.zeros(5, dtype=np.uint32), np.arange(5, dtype=np.uint32) * 1000 + 1)
    r, a, h = eng.dosage_sums()
    assert len(h) == 5 and not h.any() and not r.any() and not a.any()
    assert L.ldp_get_dosage_sums(eng._h, 4, 2, ref, alt, has) == pkg.LDP_ERR_INVALID
    eng.close()
