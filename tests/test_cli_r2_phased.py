"""plink2-hip --r2-phased / --r-phased: the .vcor table byte for byte against the reference binary's, on .bed and .pgen inputs without
phase, fully and partially phased .pgen files and a file with non-founders."""
import os
import subprocess

import numpy as np
import pytest

import ldtools as T

pytestmark = pytest.mark.gpu

M, N = 400, 150
COLS = "cols=+d,+dprime,+dprimeabs,+maj,+freq"


def _layout():
    chroms = ["2"] * 230 + ["9"] * 170
    rng = np.random.default_rng(4)
    pos = np.concatenate([np.sort(rng.choice(np.arange(1, 400000), 230, replace=False)), np.sort(rng.choice(np.arange(1, 300000), 170, replace=False))])
    return chroms, pos


def _make(kind, tmp):
    """returns the reference's / the front-end's input arguments"""
    chroms, pos = _layout()
    if kind in ("bed0", "pgen3"):
        raw = T.synth_raw_codes(M, N, seed=31, missing_rate=0.0 if kind == "bed0" else 0.03)
        raw[7] = 0          # monomorphic: never printed
        raw[8, :] = 3       # never called
        raw[9] = 1          # every sample heterozygous
        if kind == "bed0":
            T.write_bed(os.path.join(tmp, "d"), raw, chroms, pos)
            return ["--bfile", "d"]
        T.write_pgen_fixed(os.path.join(tmp, "d"), raw, chroms, pos)
        return ["--pfile", "d"]
    if kind == "phased":
        raw, present, info = T.synth_phased(M, N, seed=32, missing_rate=0.02)
        T.write_pgen_phased(os.path.join(tmp, "d"), raw, info, chroms, pos)
        return ["--pfile", "d"]
    if kind == "partial":
        raw = T.synth_raw_codes(M, N, seed=33, missing_rate=0.02)
        present, info = T.synth_phase(raw, seed=34, unphased_rate=0.3)
        T.write_vcf(os.path.join(tmp, "d.vcf"), raw, chroms, pos, present, info)
        T.ref_import_vcf(os.path.join(tmp, "d.vcf"), os.path.join(tmp, "d"))
        return ["--pfile", "d"]
    assert kind == "nonfounders"
    raw, present, info = T.synth_phased(M, N, seed=35, missing_rate=0.02)
    parents = [("s0", "s1") if (s % 5 == 4) else ("0", "0") for s in range(N)]   # every fifth sample has parents: no founder
    T.write_pgen_phased(os.path.join(tmp, "d"), raw, info, chroms, pos, parents=parents)
    return ["--pfile", "d"]


CASES = [
    ("bed0", "--r2-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
    ("bed0", "--r-phased", [], ["--ld-window-kb", "60"]),
    ("pgen3", "--r2-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
    ("pgen3", "--r2-phased", [], ["--ld-window-kb", "60"]),                                  # the default threshold 0.2
    ("pgen3", "--r-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0.5"]),
    ("pgen3", "--r2-phased", ["ref-based", "cols=+d,+dprime,+ref,+alt"], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
    ("pgen3", "--r2-phased", ["cols=+d,+dprime"], ["--ld-window-kb", "60", "--ld-window-r2", "0", "--ld-snp", "snp120"]),
    ("phased", "--r2-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
    ("phased", "--r-phased", ["cols=+d,+dprime"], ["--ld-window-kb", "60"]),
    ("phased", "--r-phased", ["ref-based", "cols=+d,+dprime"], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
    ("partial", "--r2-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
    ("partial", "--r-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0.5"]),
    ("nonfounders", "--r2-phased", [COLS], ["--ld-window-kb", "60", "--ld-window-r2", "0"]),
]


@pytest.mark.parametrize("kind,flag,mods,extra", CASES)
def test_table_is_byte_identical_to_the_reference(gpu_pkg, tmp_path, kind, flag, mods, extra):
    assert T.have_ref()
    cli = gpu_pkg.build_cli()
    tmp = str(tmp_path)
    src = _make(kind, tmp)
    ref = T.run_ref(src + [flag] + mods + extra + ["--out", "ref"], tmp)
    assert ref.returncode == 0, ref.stdout
    got = subprocess.run([cli] + src + [flag] + mods + extra + ["--out", "hip"], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert got.returncode == 0, got.stdout
    want, have = open(os.path.join(tmp, "ref.vcor")).read(), open(os.path.join(tmp, "hip.vcor")).read()
    assert want.count("\n") > 20, want[:300]
    if want != have:
        wl, hl = want.split("\n"), have.split("\n")
        bad = [(a, b) for a, b in zip(wl, hl) if a != b]
        raise AssertionError("%d vs %d lines, first difference %r" % (len(wl), len(hl), bad[:2]))
