"""ldp_get_allele_counts: the allele histogram pgen_aux1_kernel builds while it collapses a record with several ALT alleles, written out and kept per
row -- compared exactly against a numpy count of the reader's allele pairs (ldp_pgen_read_alleles) over the same samples.  Files imported from
VCF by the reference with 3, 4, 5, 6 and 19 alleles per variant (the kernel counts the first four alleles in registers, the others in LDS), dense
other-allele calls (bit-array patch sets) and a handful per variant (sample-id list patch sets); 2 to 1,025 samples, 70,001 once; through a subset
sample map, in launches of seven rows, after ldp_restrict_variants, after a reload, and not at all for a row the host built."""
import numpy as np
import pytest

import ldtools as T

pytestmark = pytest.mark.gpu

ALT_CYCLE = (1, 2, 3, 4, 5, 18)     # ALT alleles per variant: allele counts 2 (no entry), 3, 4, 5, 6 and 19
BASES = ["C", "G", "T", "AC", "AG", "AT", "ACC", "AGG", "ATT", "ACCC", "AGGG", "ATTT", "ACCCC", "AGGGG", "ATTTT", "ACCCCC", "AGGGGG", "ATTTTT"]


def write_vcf(path, m, n, seed):
    """variant v has ALT_CYCLE[v % 6] ALT alleles; the second round of the cycle (and every other one) names its later alleles in a handful of
    samples only, which the reference's writer stores as sample-id lists, the others all over the row (bit arrays); 3 % missing calls"""
    rng = np.random.default_rng(seed)
    alt_ct = np.array([ALT_CYCLE[v % len(ALT_CYCLE)] for v in range(m)])
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=1>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"GT\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%d" % s for s in range(n)) + "\n")
        for v in range(m):
            k = int(alt_ct[v])
            if (v // len(ALT_CYCLE)) % 2 == 0:
                w = rng.dirichlet(np.ones(k + 1) * (0.6 if v % 3 else 2.0))
                a, b = rng.choice(k + 1, size=n, p=w), rng.choice(k + 1, size=n, p=w)
            else:
                a, b = (rng.random(n) < 0.4).astype(np.int64), (rng.random(n) < 0.4).astype(np.int64)
                rare = rng.choice(n, size=min(n, 5), replace=False)
                a[rare] = rng.integers(0, k + 1, size=rare.size)
                b[rare] = rng.integers(max(k - 1, 0), k + 1, size=rare.size)
            l, h = np.minimum(a, b), np.maximum(a, b)
            miss = rng.random(n) < 0.03
            gts = np.where(miss, "./.", np.char.add(np.char.add(l.astype(str), "/"), h.astype(str)))
            f.write("1\t%d\tsnp%d\tA\t%s\t.\t.\t.\tGT\t%s\n" % (1000 + 37 * v, v, ",".join(BASES[:k]), "\t".join(gts)))
    return alt_ct


_files = {}


@pytest.fixture(scope="module")
def filedir(tmp_path_factory):
    assert T.have_ref(), "needs the reference binary (oracle/_ref/plink2): it imports the VCFs"
    return tmp_path_factory.mktemp("allele_counts")


def fileset(pkg, filedir, n, m):
    """(PgenFile, alt_ct, want): want[v] = the whole file's count of every allele of variant v, from the reader's pairs; made once per shape"""
    if (n, m) not in _files:
        tag = "n%d" % n
        alt_ct = write_vcf(str(filedir / (tag + ".vcf")), m, n, seed=n)
        cp = T.run_ref(["--vcf", tag + ".vcf", "--make-pgen", "--out", tag], str(filedir))
        assert cp.returncode == 0, cp.stdout[-800:]
        f = pkg.PgenFile(str(filedir / (tag + ".pgen")))
        pairs = [f.read_alleles(v, int(alt_ct[v])) for v in range(m)]
        _files[(n, m)] = (f, alt_ct, pairs)
    return _files[(n, m)]


def count(pairs, alt_ct, samples=None):
    lo, hi = pairs
    if samples is not None:
        lo, hi = lo[samples], hi[samples]
    called = lo != 255
    cnt = np.zeros(alt_ct + 1, dtype=np.int64)
    np.add.at(cnt, lo[called], 1)
    np.add.at(cnt, hi[called], 1)
    return cnt


def matrix_engine(pkg, n, m):
    eng = pkg.LdPruneEngine(max(n, 2), 40, 1, False, 0.3, order=2, device=0)
    eng.set_variants_matrix(m)
    return eng


def widths(alt_ct):
    return np.where(alt_ct > 1, alt_ct + 1, 0)


def check(eng, alt_ct, pairs, variants, samples=None, first=0):
    """the engine's variants [first, first + len(variants)) hold the file's `variants`"""
    got, has = eng.allele_counts(widths(alt_ct[variants]), first)
    for q, v in enumerate(variants):
        if alt_ct[v] > 1:
            assert has[q] == 1, v
            assert np.array_equal(got[q].astype(np.int64), count(pairs[v], int(alt_ct[v]), samples)), (v, got[q], count(pairs[v], int(alt_ct[v]), samples))
        else:
            assert has[q] == 0 and got[q].size == 0, v


@pytest.mark.parametrize("n,m", [(2, 24), (63, 36), (64, 36), (65, 36), (257, 36), (1025, 36), (70001, 12)])
def test_counts_are_the_readers(gpu_pkg, filedir, n, m):
    f, alt_ct, pairs = fileset(gpu_pkg, filedir, n, m)
    assert set((alt_ct + 1).tolist()) == {2, 3, 4, 5, 6, 19}
    # alleles beyond the fourth are named somewhere (they take the LDS histogram, not the registers), unless the file is tiny
    assert n < 63 or any(count(pairs[v], int(alt_ct[v]))[4:].sum() > 0 for v in range(m) if alt_ct[v] >= 4)
    eng = matrix_engine(gpu_pkg, n, m)
    maj = eng.load_pgen_records(0, f, allele_cts=alt_ct + 1)
    check(eng, alt_ct, pairs, np.arange(m))
    # the counts are the ones the major allele was chosen from
    for v in range(m):
        if alt_ct[v] > 1:
            assert maj[v] == T.major_allele_multi(count(pairs[v], int(alt_ct[v])))[0], v
    # a slot of another width than the row's allele count gets nothing
    wrong = widths(alt_ct) + (alt_ct > 1)
    got, has = eng.allele_counts(wrong)
    assert not has.any() and all((g == 0).all() for g in got)
    eng.close()


@pytest.mark.parametrize("n,m", [(65, 36), (1025, 36)])
def test_counts_run_over_a_subset_sample_map(gpu_pkg, filedir, n, m):
    f, alt_ct, pairs = fileset(gpu_pkg, filedir, n, m)
    keep = np.flatnonzero(np.random.default_rng(n).random(n) < 0.4).astype(np.uint32)
    assert any((count(pairs[v], int(alt_ct[v]), keep) != count(pairs[v], int(alt_ct[v]))).any() for v in range(m) if alt_ct[v] > 1)
    eng = matrix_engine(gpu_pkg, len(keep), m)
    eng.set_sample_map(n, keep)
    eng.load_pgen_records(0, f, allele_cts=alt_ct + 1)
    check(eng, alt_ct, pairs, np.arange(m), samples=keep)
    eng.close()


@pytest.mark.parametrize("n,m", [(64, 36), (257, 36)])
def test_launches_of_seven_rows(gpu_pkg, filedir, n, m):
    f, alt_ct, pairs = fileset(gpu_pkg, filedir, n, m)
    eng = matrix_engine(gpu_pkg, n, m)
    eng.set_option("decode_rows", 7)
    eng.load_pgen_records(0, f, allele_cts=alt_ct + 1)
    check(eng, alt_ct, pairs, np.arange(m))
    eng.close()


@pytest.mark.parametrize("n,m", [(63, 36), (1025, 36)])
def test_counts_follow_rows_through_restrict_and_are_replaced_by_a_reload(gpu_pkg, filedir, n, m):
    pkg = gpu_pkg
    f, alt_ct, pairs = fileset(pkg, filedir, n, m)
    eng = matrix_engine(pkg, n, m)
    eng.load_pgen_records(0, f, allele_cts=alt_ct + 1)
    # a reload of rows 6.. from the records of variants 2..: the rows' entries are the new records'
    eng.load_pgen_records(6, f, 2, 10, allele_cts=(alt_ct + 1)[2:12])
    now = np.concatenate([np.arange(6), np.arange(2, 12), np.arange(16, m)])
    check(eng, alt_ct, pairs, now)
    # a row the host builds has no counts: the caller counts the reader's pairs itself
    host_row = 9
    assert alt_ct[now[host_row]] > 1
    codes = np.zeros((1, n), dtype=np.uint8)
    eng.load_genotypes_host(host_row, np.ascontiguousarray(T.pack_2bit(codes).view(np.uint8).reshape(1, -1)[:, :(n + 3) // 4]), pkg.LDP_GENO_INVERSE)
    got, has = eng.allele_counts(widths(alt_ct[now]))
    assert has[host_row] == 0 and (got[host_row] == 0).all() and has[np.flatnonzero(alt_ct[now] > 1)].sum() == (alt_ct[now] > 1).sum() - 1
    # ... and the others travel with their rows when variants are dropped
    keep = np.ones(m, dtype=bool)
    keep[[0, 1, 7, 8, host_row, 20, m - 1]] = False
    eng.restrict_variants(keep, np.zeros(int(keep.sum()), dtype=np.uint32), (np.arange(int(keep.sum()), dtype=np.uint32) + 1) * 1000)
    check(eng, alt_ct, pairs, now[keep])
    # a new plan clears them
    eng.set_variants_matrix(m)
    got, has = eng.allele_counts(widths(alt_ct))
    assert not has.any()
    eng.close()


def test_rows_of_a_fixed_width_file_have_no_counts(gpu_pkg):
    pkg = gpu_pkg
    m, n = 20, 70
    raw = T.synth_raw_codes(m, n, seed=2, missing_rate=0.02)
    eng = matrix_engine(pkg, n, m)
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
    got, has = eng.allele_counts(np.full(m, 3))
    assert not has.any() and all((g == 0).all() for g in got)
    eng.close()
