"""What keeps the comparisons of test_gpu_attention_dropout.py meaningful, asserted on the host replica of the draws alone
(attn_dropout_cases.py): the masks of every case there contain the rows at which a kernel can go wrong -- a row of one chunk (at
most four entries: no stored attn_out, delta rebuilt in the destination pass) with some but not all weights dropped, rows of two
and of more chunks with a drop, a dropped and a kept self entry, at p = 0.5 a (row, head) with everything and one with nothing
dropped, two heads of one pair hash that differ -- and the replica drops the stated fraction of the weights."""
import math

import numpy as np
import pytest

import attn_dropout_cases as cases


def _row_drops(ent, keep):
    """dropped[row, head]: number of dropped entries."""
    drops = np.zeros((ent.n, keep.shape[1]), dtype=np.int64)
    np.add.at(drops, ent.dst, ~keep)
    return drops


@pytest.mark.parametrize("pair_key", [False, True])
def test_graphs_are_what_the_cases_say(pair_key):
    g = cases.graph(pair_key)
    assert g.n == 300 and set(np.bincount(g.dst, minlength=g.n)) == set(cases.DEGREES)
    assert not (g.src == g.dst).any()
    pairs = g.dst * g.n + g.src
    repeated = pairs.shape[0] - np.unique(pairs).shape[0]
    assert (repeated == 0) if pair_key else (repeated > 10)
    assert set(g.loops) == ({0, 1} if pair_key else {0, 1, 2})
    in_ptr, in_src, loops, e = g.host_csr()
    ent = cases.Entries(in_ptr, in_src, loops, e)
    assert len(ent) == e + int((loops > 0).sum())
    # a row's entries: its in-entries in order, then the self entry at E + row
    for i in (0, 7, 150, 299):
        a, c = ent.first[i], ent.count[i]
        want = list(range(in_ptr[i], in_ptr[i + 1])) + ([e + i] if loops[i] > 0 else [])
        assert ent.pos[a:a + c].tolist() == want and (ent.dst[a:a + c] == i).all()
        assert ent.mult[a:a + c].tolist() == [1] * (c - (loops[i] > 0)) + ([loops[i]] if loops[i] > 0 else [])


@pytest.mark.parametrize("pair_key,heads,p,counter", cases.mask_cases())
def test_masks_of_the_per_edge_cases_contain_the_rows_that_matter(pair_key, heads, p, counter):
    ent, keep = cases.host_mask(pair_key, heads, p, counter)
    drops = _row_drops(ent, keep)
    cnt = ent.count[:, None]
    some = (drops > 0) & (drops < cnt)
    assert (some & (cnt <= 4)).any(), "no row of one chunk with some but not all weights dropped"
    assert ((drops > 0) & (cnt >= 5) & (cnt <= 8)).any(), "no row of two chunks with a drop"
    assert ((drops > 0) & (cnt > 8)).any(), "no row of more than two chunks with a drop"
    selfs = keep[ent.is_self]
    assert (~selfs).any() and selfs.any(), "self entries: a dropped and a kept one"
    if p == 0.5:
        assert ((drops == cnt) & (cnt > 0)).any(), "no (row, head) with every weight dropped"
        assert ((drops == 0) & (cnt > 0)).any(), "no (row, head) with every weight kept"
    if pair_key and heads >= 2:
        assert (keep[:, 0] != keep[:, 1]).any(), "the two 16-bit fields of one hash give the same draws"
    # the stated fraction: within four standard deviations of a binomial of M draws
    m = keep.size
    assert abs((~keep).mean() - p) < 4.0 * math.sqrt(p * (1.0 - p) / m), ((~keep).mean(), m)


@pytest.mark.parametrize("pair_key", [False, True])
@pytest.mark.parametrize("p", cases.PS)
def test_the_replica_drops_the_stated_fraction(pair_key, p):
    """n = 300, H = 3: more than 5000 draws."""
    _, keep = cases.host_mask(pair_key, 3, p)
    m = keep.size
    assert m >= 5000
    frac = (~keep).mean()
    assert abs(frac - p) < 4.0 * math.sqrt(p * (1.0 - p) / m), (frac, m)


@pytest.mark.parametrize("heads,ch,p,loops_p", cases.DENSE_CASES)
def test_masks_of_the_dense_block_cases_contain_the_rows_that_matter(heads, ch, p, loops_p):
    """The blocky graphs have rows of 0-4 and of 60+ entries only (no row of two chunks); with loops_p = 1 every row has a self
    entry."""
    g = cases.blocky_graph(cases.dense_graph_seed(heads), loops_p)
    in_ptr, in_src, loops, e = g.host_csr()
    ent = cases.Entries(in_ptr, in_src, loops, e)
    keep = cases.mask(in_ptr, in_src, loops, e, heads, p, cases.DROP_SEED, None, True)
    pairs = g.dst * g.n + g.src
    assert np.unique(pairs).shape[0] == pairs.shape[0] and not (g.src == g.dst).any()
    drops = _row_drops(ent, keep)
    cnt = ent.count[:, None]
    assert ((drops > 0) & (drops < cnt) & (cnt <= 4)).any()
    assert ((drops > 0) & (cnt >= 32)).any()
    selfs = keep[ent.is_self]
    assert (~selfs).any() and selfs.any()
    assert (keep[:, 0] != keep[:, 1]).any()
    m = keep.size
    assert m >= 5000 and abs((~keep).mean() - p) < 4.0 * math.sqrt(p * (1.0 - p) / m)


def test_the_blocky_graphs_are_those_of_the_dense_block_tests():
    """attn_dropout_cases.blocky_graph restates the host part of test_gpu_dense_blocks._make (which builds its structure on the
    device as it goes): same edges and self entries for one seed, so the two cannot drift apart unnoticed."""
    import test_gpu_dense_blocks as dense

    assert dense.SIZES == cases.BLOCK_SIZES
    ei, loops, n = dense._blocky_graphs(np.random.RandomState(13), dense.SIZES, 0.3)
    g = cases.blocky_graph(13, 0.3)
    assert n == g.n and (ei[0] == g.src).all() and (ei[1] == g.dst).all() and (loops == g.loops).all()


def test_the_seed_counter_mix():
    seed = cases.DROP_SEED
    assert cases.mixed_seed(seed) == seed and cases.mixed_seed(seed, 0) == seed
    assert cases.mixed_seed(seed, 3) == (seed + 3 * 0xD1B54A32D192ED03) % 2 ** 64 != seed
    assert cases.mixed_seed(2 ** 64 - 1, 1) == 0xD1B54A32D192ED03 - 1            # wraps
    assert cases.mixed_seed(-1) == 2 ** 64 - 1                                   # as the launchers pass a Python int: masked
    for pair_key in (False, True):
        _, plain = cases.host_mask(pair_key, 3, 0.1)
        _, at0 = cases.host_mask(pair_key, 3, 0.1, 0)
        _, at3 = cases.host_mask(pair_key, 3, 0.1, 3)
        assert (plain == at0).all() and (plain != at3).any()


def test_the_draws_in_numbers():
    """The pieces of the replica: the hash against a second spelling, the thresholds, which half of a pair hash a head reads, the
    high word of a 64-bit index."""
    assert cases.avalanche32(0) == 0
    assert cases.avalanche32(1) == _avalanche32_spelt_out(1)
    assert cases.pair_threshold(0.1) == 6553 and cases.pair_threshold(0.5) == 32768
    # an index above 2^32 reaches the second round through its high word
    assert cases.uniform01_edge(5, 7) != cases.uniform01_edge(5, 7 + (1 << 32))
    u = cases.uniform01_edge(5, 7)
    assert u.dtype == np.float32 and 0.0 <= u < 1.0
    # the two heads of a pair read the low and the high half of ONE hash
    hsh = cases.pair_hash(9, 4, 2, 0)
    thr = cases.pair_threshold(0.5)
    assert cases.pair_dropped(9, 4, 2, 0, 0.5) == ((hsh & 0xFFFF) < thr)
    assert cases.pair_dropped(9, 4, 2, 1, 0.5) == ((hsh >> 16) < thr)
    assert cases.pair_hash(9, 4, 2, 1) != hsh and cases.pair_hash(9, 2, 4, 0) != hsh


def _avalanche32_spelt_out(x):
    x = (x ^ (x >> 16)) * 0x7FEB352D % 2 ** 32
    x = (x ^ (x >> 15)) * 0x846CA68B % 2 ** 32
    return x ^ (x >> 16)
