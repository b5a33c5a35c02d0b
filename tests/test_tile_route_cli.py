"""plink2-hip on a fileset whose missingness differs along the genome: the prune lists byte-identical to the reference binary, and the
--timing line of the per-tile routes names tiles of all three classes."""
import filecmp
import re

import pytest

import ldtools as T
import tile_route_tools as R
from test_cli import cli, run_cli   # noqa: F401  (the fixture that builds the front-end)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bfile", "pfile"])
def test_cli_stretches_byte_identical_and_three_classes(gpu_pkg, cli, tmp_path, fmt):
    assert T.have_ref(), "reference binary oracle/_ref/plink2 must travel with the repo snapshot"
    m, second, n = 1800, 200, 300
    raw, chr_idx = R.stretch_rows(m, n, seed=4600, stretches=[(300, 600, 0.05), (1300, 1400, 0.001)], second=second)
    chroms = [str(int(c) + 1) for c in chr_idx]
    bps = [1000 + 100 * (v if v < m else v - m) for v in range(m + second)]
    prefix = str(tmp_path / "d")
    if fmt == "bfile":
        T.write_bed(prefix, raw, chroms, bps)
    else:
        T.write_pgen_fixed(prefix, raw, chroms, bps)
    common = ["--" + fmt, "d", "--indep-pairwise", "600", "1", "0.2"]
    ref = T.run_ref(common + ["--threads", "4", "--out", "ref"], str(tmp_path))
    assert ref.returncode == 0, ref.stdout
    got = run_cli(cli, common + ["--timing", "--out", "hip"], str(tmp_path))
    assert got.returncode == 0, got.stdout
    assert filecmp.cmp(str(tmp_path / "ref.prune.in"), str(tmp_path / "hip.prune.in"), shallow=False)
    assert filecmp.cmp(str(tmp_path / "ref.prune.out"), str(tmp_path / "hip.prune.out"), shallow=False)
    assert "[timing] pair launches by route: complete data 0 | a few missing calls 0 " in got.stdout, got.stdout
    line = re.search(r"\[timing\] tiles by their own rows: complete data (\d+) \| a few missing calls (\d+) \| missing calls (\d+) \(quarter tiles\) \| (\d+) corner products handed over",
                     got.stdout)
    assert line, got.stdout
    complete, sparse, general, corners = (int(x) for x in line.groups())
    assert complete > 0 and sparse > 0 and general > 0 and corners > 0
    tiles = int(re.search(r"(\d+) tiles planned", got.stdout).group(1))
    assert complete + sparse + general == tiles
