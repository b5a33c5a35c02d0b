#!/usr/bin/env python3
"""Config 3's density slice of bench.py (500,000 samples x --variants at 290 bp, `500kb 0.2`) with missingness that DIFFERS ALONG THE GENOME,
stepped with per-tile routing on and off (engine option "tile_route" 1 / 0, alternating in one process after a warm-up).
The image is generated stretch by stretch: the generator takes a missing-call rate per call and a genotype is a pure function of (seed,
variant, sample), so a stretch generated again at another rate is the same rows with calls knocked out.

Layouts (--layouts a,b,c,d):
  a  complete
  b  3 % of the variants at 5 % missing, in stretches of 2,048
  c  the first 2,048 variants at 0.1 %, the rest complete
  d  3 % of the variants at 5 % missing, scattered one by one (every tile holds some: nothing to gain, recorded anyway)
Per layout and option: ms per step (each step listed), the pair kernels' ms, the launches by route word, the tiles by class, and whether
the prune sets of the two options are identical.  One JSON line.  An engine without the option (an older library) is stepped as "0" only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import __graft_entry__ as ge  # noqa: E402

STRETCH = 2048


def stretches_of(layout, m):
    """[(first variant, variants, missing rate)]"""
    if layout == "a":
        return []
    if layout == "c":
        return [(0, min(STRETCH, m), 0.001)]
    want = int(0.03 * m)
    rng = np.random.default_rng(12)
    if layout == "b":
        k = max(1, round(want / STRETCH))
        slots = np.sort(rng.choice(m // STRETCH, size=k, replace=False))
        return [(int(s) * STRETCH, STRETCH, 0.05) for s in slots]
    if layout == "d":
        return [(int(v), 1, 0.05) for v in np.sort(rng.choice(m, size=want, replace=False))]
    raise SystemExit("unknown layout " + layout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=120000)
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--layouts", default="a,b,c,d")
    ap.add_argument("--steps", type=int, default=3, help="timed steps per option (alternating 1, 0, 1, 0, ..)")
    ap.add_argument("--package", default=None, help="directory of another build of the package (a parent commit's, to confirm that option 0 equals it)")
    args = ap.parse_args()
    import torch
    if args.package:
        import importlib.util
        pkg_dir = os.path.abspath(args.package)
        spec = importlib.util.spec_from_file_location("plink_ng_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
        pkg = importlib.util.module_from_spec(spec)
        sys.modules["plink_ng_amd"] = pkg
        spec.loader.exec_module(pkg)
    else:
        pkg = ge.load_package()
    has_option = hasattr(pkg.LdPruneEngine, "tile_routes")
    cfg = dict(bench.CONFIGS["config3"])
    cfg["variants"] = args.variants
    if args.samples:
        cfg["samples"] = args.samples
    out = {"samples": cfg["samples"], "variants": cfg["variants"], "window_kb": cfg["window_kb"], "r2": cfg["r2"], "library": pkg.LIB_PATH,
           "tile_route_option": has_option, "layouts": {}}
    for layout in args.layouts.split(","):
        w = bench.Workload(pkg, torch, cfg, 0.0, 0, 1, 0, {}, None)
        assert w.resident and len(w.engines) == 1
        eng = w.engines[0][0]
        st = stretches_of(layout, cfg["variants"])
        for first, ln, rate in st:
            for seg_first, seg_ln, ptr, stride in w.segs[id(eng)]:
                a, b = max(first, seg_first), min(first + ln, seg_first + seg_ln)
                if a < b:
                    pkg.synth_genotypes_device(bench.SEED, a, b - a, w.founder_ct, rate, ptr + (a - seg_first) * stride, stride)
        torch.cuda.synchronize()
        options = (1, 0) if has_option else (0,)
        res = {str(o): {"ms_per_step": [], "pair_kernels_ms": []} for o in options}
        words_of = {}
        for rep in range(args.steps + 1):  # (rep 0: the warm-up of both options)
            for o in options:
                if has_option:
                    eng.set_option("tile_route", o)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                words, cc = w.step()
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                c = cc[0]
                r = res[str(o)]
                if rep:
                    r["ms_per_step"].append(1e3 * el)
                    r["pair_kernels_ms"].append(c["ms_pair_kernel"])
                r["routes"] = {"complete": c["route_complete_launches"], "sparse": c["route_sparse_launches"], "general": c["route_general_launches"]}
                r["four_tile_launches"], r["sparse_tile_launches"], r["wide_tiles"] = c["four_tile_launches"], c["sparse_tile_launches"], c["wide_tiles"]
                r["pred_true"], r["candidate_pairs"], r["pairs_counted_exactly"] = c["pred_true"], c["candidate_pairs"], c["sparse_exact_pairs"]
                r["tiles"] = eng.tile_routes() if has_option else None
                r["variants_removed"] = int(np.unpackbits(np.asarray(words).view(np.uint8)).sum())
                if str(o) in words_of:
                    r["same_as_own_first_step"] = bool(np.array_equal(words_of[str(o)], words)) and r.get("same_as_own_first_step", True)
                else:
                    words_of[str(o)] = np.array(words, copy=True)
        for o in options:
            r = res[str(o)]
            r["ms_per_step_mean"] = float(np.mean(r["ms_per_step"]))
            r["pair_kernels_ms_mean"] = float(np.mean(r["pair_kernels_ms"]))
        res["stretches"] = len(st)
        res["variants_with_missing_calls"] = int(sum(ln for _, ln, _ in st))
        res["prune_sets_identical"] = bool(all(np.array_equal(words_of[str(options[0])], words_of[str(o)]) for o in options[1:]))
        import hashlib
        res["prune_set_sha1"] = hashlib.sha1(np.ascontiguousarray(words_of[str(options[0])]).tobytes()).hexdigest()
        out["layouts"][layout] = res
        w.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
