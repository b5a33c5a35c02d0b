"""plink2-hip --indep-pairwise on a file with dosage tracks: the allele frequencies -- hence the major allele and the tie-break of which
variant of a correlated pair goes -- come from the dosage sums (plink2_data.cc:2421-2443), and those from the load's own decode
(pgen_dosage_kernel -> ldp_get_dosage_sums) instead of a second read of the file on the host.  Lists against the reference's and
against plink2-hip's host pass (--debug-host-decode), on a fileset the reference's --dummy wrote; the --timing line says where the
sums came from."""
import filecmp
import os
import re

import pytest

import ldtools as T
from test_cli import cli, run_cli  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PRUNE = ["--indep-pairwise", "100", "5", "0.1"]
LINE = re.compile(r"allele frequencies of (\d+) variants from their dosages: (\d+) summed on the device by the load, (\d+) by the host pass")


@pytest.fixture(scope="module")
def dosage_dir(tmp_path_factory):
    if not T.have_ref():
        pytest.skip("oracle/_ref/plink2 not built (it writes the fileset)")
    d = tmp_path_factory.mktemp("cli_dosage_device")
    cp = T.run_ref(["--dummy", "300", "400", "dosage-freq=0.4", "--seed", "3", "--threads", "2", "--make-pgen", "--out", "dos"], str(d))
    assert cp.returncode == 0, cp.stdout[-800:]
    # the same genotypes with every fifth sample a child of two others: founders among non-founders
    psam = open(str(d / "dos.psam")).read().splitlines()
    assert psam[0].split("\t")[:2] == ["#IID", "SEX"]
    out = ["#IID\tPAT\tMAT\tSEX"]
    for k, line in enumerate(psam[1:]):
        iid, sex = line.split("\t")[:2]
        out.append("\t".join([iid, "per1", "per2", sex] if (k % 5 == 4) else [iid, "0", "0", sex]))
    open(str(d / "nf.psam"), "w").write("\n".join(out) + "\n")
    for ext in (".pgen", ".pvar"):
        os.link(str(d / ("dos" + ext)), str(d / ("nf" + ext)))
    # ... and with the second half of the variants on another chromosome: two subcontigs, one per engine under --gpus 2
    pvar = open(str(d / "dos.pvar")).read().splitlines()
    body = [l for l in pvar if not l.startswith("#")]
    assert len(body) == 400
    moved = [l if k < 200 else "\t".join(["2"] + l.split("\t")[1:]) for k, l in enumerate(body)]
    open(str(d / "two.pvar"), "w").write("\n".join([l for l in pvar if l.startswith("#")] + moved) + "\n")
    for ext in (".pgen", ".psam"):
        os.link(str(d / ("dos" + ext)), str(d / ("two" + ext)))
    return d


def counts(stdout):
    hit = LINE.search(stdout)
    assert hit, stdout[-1500:]
    return tuple(int(x) for x in hit.groups())


def same_lists(cwd, a, b):
    for ext in (".prune.in", ".prune.out"):
        assert filecmp.cmp(os.path.join(cwd, a + ext), os.path.join(cwd, b + ext), shallow=False), (a, b, ext)


@pytest.mark.parametrize("name,extra", [("dos", []), ("nf", []), ("two", ["--gpus", "2", "--debug-alias-devices"])], ids=["founders", "non-founders", "two-engines"])
def test_lists_match_the_reference_and_the_host_pass(gpu_pkg, cli, dosage_dir, name, extra):
    cwd = str(dosage_dir)
    tag = name
    args = ["--pfile", name] + PRUNE
    ref = T.run_ref(args + ["--threads", "4", "--out", tag + "_ref"], cwd)
    dev = run_cli(cli, args + extra + ["--timing", "--out", tag + "_dev"], cwd)
    host = run_cli(cli, args + extra + ["--timing", "--debug-host-decode", "--out", tag + "_host"], cwd)
    assert ref.returncode == 0 and dev.returncode == 0 and host.returncode == 0, (ref.stdout[-600:], dev.stdout[-1500:], host.stdout[-1500:])
    same_lists(cwd, tag + "_ref", tag + "_dev")
    same_lists(cwd, tag + "_ref", tag + "_host")
    listed = [len(open(os.path.join(cwd, tag + "_ref" + e)).read().split()) for e in (".prune.in", ".prune.out")]
    assert sum(listed) == 400 and min(listed) > 20, listed       # (the prune removes something and leaves something)
    total, device, host_ct = counts(dev.stdout)
    assert total > 200 and device == total and host_ct == 0, dev.stdout[-1500:]
    assert counts(host.stdout) == (total, 0, total), host.stdout[-1500:]
