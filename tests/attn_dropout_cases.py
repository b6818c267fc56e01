"""What the attention-dropout tests share (test_attn_dropout_cpu.py, test_gpu_attention_dropout.py): a host replica of the two
dropout draws of TransformerConv's attention kernels, an fp64 reference of the edge softmax with a given mask, the graphs and the
list of cases.  numpy and torch on the CPU only; no tests in here.

The draws (csrc/attn_fwd.hpp: attn_drop_key, attn_pair_hash, attn_pair_dropped; csrc/common.hpp: avalanche32, uniform01_edge), in
Python integers:

  * position key: the weight at in-CSR position ``pos`` (the self entry of row i: ``E + i``) of head h is dropped when
    uniform01_edge(seed', pos * H + h) < p, the uniform being (x >> 8) * 2^-24 of a 32-bit hash x, compared in float32 (both sides
    are float32 numbers, the product by 2^-24 is exact: no margin);
  * pair key: heads 2k and 2k + 1 of (destination, source) share the 32-bit hash attn_pair_hash(seed', dst, src, k); head h is
    dropped when its 16-bit field (h & 1) is below floor(float32(p) * 65536);
  * seed' = seed + counter * 0xD1B54A32D192ED03 (mod 2^64) when a step counter is installed, else seed.

An ENTRY of row i is one of its CSR in-entries, in the order of the structure's in_ptr / in_src, or -- last, if loops[i] > 0 -- its
self entry, ONE entry (one draw) of weight loops[i] whatever the multiplicity.
"""
import functools

import numpy as np
import torch

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
COUNTER_MIX = 0xD1B54A32D192ED03


# ------------------------------------------------------------------------------------------------ the draws
def mixed_seed(seed, counter=None):
    """The seed a kernel draws with: ``counter`` is the value of the installed device counter (None: none installed)."""
    seed &= M64
    return seed if counter is None else (seed + counter * COUNTER_MIX) & M64


def avalanche32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def uniform01_edge(seed, idx):
    """common.hpp uniform01_edge as a float32."""
    x = avalanche32((idx & M32) ^ (seed & M32))
    x = avalanche32(x ^ (seed >> 32) ^ (((idx >> 32) * 0x9E3779B1) & M32))
    return np.float32(x >> 8) * np.float32(2.0 ** -24)


def position_dropped(seed, pos, heads, h, p):
    return bool(uniform01_edge(seed, pos * heads + h) < np.float32(p))


def pair_hash(seed, dst, src, hpair):
    x = avalanche32((src & M32) ^ (seed & M32))
    return avalanche32(x ^ (seed >> 32) ^ ((dst * 0x9E3779B1) & M32) ^ ((hpair * 0x85EBCA6B) & M32))


def pair_threshold(p):
    return int(np.float32(p) * np.float32(65536.0))


def pair_dropped(seed, dst, src, h, p):
    return ((pair_hash(seed, dst, src, h >> 1) >> (16 * (h & 1))) & 0xFFFF) < pair_threshold(p)


# ------------------------------------------------------------------------------------------------ entries and masks
class Entries:
    """The entries of every row, row after row: ``dst`` / ``src`` (the self entry: src = dst), ``pos`` (in-CSR position; the self
    entry of row i: E + i), ``mult`` (weight of the entry inside the softmax: 1, the self entry loops[i]), ``is_self``, and per row
    ``count`` and ``first`` (the row's entries are first[i] .. first[i] + count[i] - 1)."""

    def __init__(self, in_ptr, in_src, loops, num_edges):
        in_ptr, in_src, loops = (np.asarray(a).astype(np.int64) for a in (in_ptr, in_src, loops))
        n, e = loops.shape[0], int(num_edges)
        assert in_ptr[n] == e
        deg = np.diff(in_ptr[:n + 1])
        rows_self = np.nonzero(loops > 0)[0]
        dst = np.concatenate([np.repeat(np.arange(n), deg), rows_self])
        src = np.concatenate([in_src[:e], rows_self])
        pos = np.concatenate([np.arange(e), e + rows_self])
        mult = np.concatenate([np.ones(e, np.int64), loops[rows_self]])
        is_self = np.concatenate([np.zeros(e, bool), np.ones(rows_self.shape[0], bool)])
        order = np.lexsort((pos, dst))              # by row; inside a row by position: the self entry (pos >= E) last
        self.dst, self.src, self.pos, self.mult, self.is_self = dst[order], src[order], pos[order], mult[order], is_self[order]
        self.n, self.num_edges = n, e
        self.count = deg + (loops > 0)
        self.first = np.concatenate([[0], np.cumsum(self.count)[:-1]])

    def __len__(self):
        return self.dst.shape[0]


def mask(in_ptr, in_src, loops, num_edges, heads, p, seed, counter, pair_key):
    """keep[entry, head] (False: the weight is dropped) for the entries of ``Entries(in_ptr, in_src, loops, num_edges)``."""
    ent = Entries(in_ptr, in_src, loops, num_edges)
    s = mixed_seed(seed, counter)
    keep = np.ones((len(ent), heads), dtype=bool)
    thr = pair_threshold(p)
    for x, (d, j, pos) in enumerate(zip(ent.dst.tolist(), ent.src.tolist(), ent.pos.tolist())):
        for h in range(heads):
            if not pair_key:
                keep[x, h] = not position_dropped(s, pos, heads, h, p)
            else:
                if h % 2 == 0:                      # one hash for heads h and h + 1
                    hash32 = pair_hash(s, d, j, h >> 1)
                keep[x, h] = ((hash32 >> (16 * (h & 1))) & 0xFFFF) >= thr
    return keep


# ------------------------------------------------------------------------------------------------ fp64 reference
def attention_fp64(q, k, v, skip, ent, keep, p):
    """TransformerConv's edge softmax on [n, H, C] float64 operands (differentiable): scores q . k / sqrt(C), softmax over a row's
    entries with the self entry weighted by its multiplicity and 1e-16 added to the denominator, THEN alpha * keep / (1 - p), the
    weighted sum of the value rows, + skip.  The mask is a constant.  Returns [n, H C]."""
    n, heads, ch = q.shape
    dst, src = torch.from_numpy(ent.dst), torch.from_numpy(ent.src)
    score = (q[dst] * k[src]).sum(-1) / ch ** 0.5                                                  # [entries, H]
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64).scatter_reduce(
        0, dst[:, None].expand(-1, heads), score.detach(), "amax")
    w = torch.exp(score - mx[dst]) * torch.from_numpy(ent.mult).double()[:, None]
    denom = torch.zeros(n, heads, dtype=torch.float64).index_add(0, dst, w) + 1e-16
    alpha = w / denom[dst]
    alpha = alpha * torch.from_numpy(keep).double() / (1.0 - p)
    agg = torch.zeros(n, heads, ch, dtype=torch.float64).index_add(0, dst, alpha[:, :, None] * v[src])
    return (agg + skip).reshape(n, heads * ch)


def reference(qkvs, gout, ent, keep, heads, ch, p):
    """(out [n, H C], gradient of qkvs [n, 4 H C]) in fp64 for compact qkvs = [query | key | value | skip] and a given ``gout``."""
    n, hc = qkvs.shape[0], heads * ch
    x = qkvs.double().requires_grad_(True)
    q, k, v, skip = (x[:, i * hc:(i + 1) * hc].reshape(n, heads, ch) for i in range(4))
    out = attention_fp64(q, k, v, skip, ent, keep, p)
    out.backward(gout.double())
    return out.detach(), x.grad


# ------------------------------------------------------------------------------------------------ graphs
N_ROWS = 300
DEGREES = [0, 1, 2, 3, 4, 5, 8, 9, 17, 40]
GRAPH_SEED = {False: 20, True: 21}         # by pair_key; chosen so that every case's mask meets test_attn_dropout_cpu.py
DROP_SEED = 0x1234_5678_9ABC_DEF1          # a seed with both halves set
COUNTER = 3


class Graph:
    """``src`` / ``dst``: the stored edges (no self-loops), ``loops`` [n]: multiplicity of every row's self entry."""

    def __init__(self, src, dst, loops, n, sizes=None, order=None, max_span=None):
        self.src, self.dst, self.loops, self.n = src.astype(np.int64), dst.astype(np.int64), loops.astype(np.int64), int(n)
        self.sizes, self.order, self.max_span = sizes, order, max_span

    def edge_index(self):
        """[2, E'] with the self-loops listed ``loops[i]`` times, what GraphStructure.from_edge_index takes."""
        selfs = np.repeat(np.stack([np.arange(self.n)] * 2), self.loops, axis=1)
        return np.concatenate([np.stack([self.src, self.dst]), selfs], axis=1)

    def host_csr(self):
        """(in_ptr, in_src, loops, E): the sources of a row in the order they were generated.  A structure built on the device may
        order them otherwise: the position key's draws do not depend on which source sits at a position, the pair key's not on
        the position, so every statement about WHICH (row, head) draws what holds for either order."""
        order = np.argsort(self.dst, kind="stable")
        in_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.dst, minlength=self.n))])
        return in_ptr, self.src[order], self.loops, self.src.shape[0]


@functools.lru_cache(maxsize=None)
def graph(pair_key):
    """n = 300 rows of 0-40 in-edges.  Position key: sources drawn with replacement (repeated edges), self entries of multiplicity
    0 / 1 / 2.  Pair key: distinct sources per row (parallel edges would share a draw there by design), multiplicity 0 / 1."""
    rng = np.random.RandomState(GRAPH_SEED[pair_key])
    n = N_ROWS
    deg = rng.choice(DEGREES, size=n)
    dst = np.repeat(np.arange(n), deg)
    if pair_key:
        src = np.concatenate([rng.choice(n - 1, size=d, replace=False) for d in deg])
        src = np.where(src >= dst, src + 1, src)                        # never the row itself
        loops = rng.randint(0, 2, size=n)
    else:
        src = rng.randint(0, n, size=dst.shape[0])
        src = np.where(src == dst, (src + 1) % n, src)                  # self-loops are the structure's own entry
        loops = rng.randint(0, 3, size=n)
    return Graph(src, dst, loops, n)


# the blocky graphs of the dense-block forms (as tests/test_gpu_dense_blocks.py builds them): long rows that share their sources
BLOCK_SIZES = [700, 1, 333, 64, 2, 1500]


@functools.lru_cache(maxsize=None)
def blocky_graph(seed, loops_p):
    """Per graph a few hubs, each with a window of ids; a row is short (0-3 sources) or long (60-200 sources of one hub's window); no
    parallel edges; self entries of multiplicity 1 with probability ``loops_p``.  ``order``: a graph's rows sorted by where their
    sources sit (rows around one hub follow each other), the last graph's rows in no order (its blocks outgrow the capacity and stay
    with the per-edge kernels)."""
    rng = np.random.RandomState(seed)
    sizes = BLOCK_SIZES
    src, dst, off = [], [], 0
    for n in sizes:
        hubs = max(1, n // 150)
        for i in range(n):
            hub = rng.randint(hubs)
            lo = hub * n // hubs
            win = np.arange(lo, min(n, lo + max(40, min(320, n // hubs + 60))))
            win = win[win != i]
            d = rng.randint(60, min(200, len(win)) + 1) if rng.rand() < 0.3 and len(win) >= 60 else rng.randint(0, 4)
            picks = rng.choice(win, size=min(d, len(win)), replace=False) if len(win) and d else np.zeros(0, np.int64)
            src.append(picks + off)
            dst.append(np.full(len(picks), i + off))
        off += n
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    n = int(sum(sizes))
    loops = (rng.rand(n) < loops_p).astype(np.int64)
    centre = np.full(n, -1.0)
    sums, cnts = np.bincount(dst, weights=src, minlength=n), np.bincount(dst, minlength=n)
    centre[cnts > 0] = np.floor(sums[cnts > 0] / cnts[cnts > 0] / 40.0)
    centre += rng.rand(n) * 0.5
    offs = np.cumsum([0] + sizes[:-1])
    centre[offs[-1]:] = rng.rand(sizes[-1])
    order = np.concatenate([np.argsort(centre[o:o + k], kind="stable") + o for k, o in zip(sizes, offs)]).astype(np.int32)
    return Graph(src, dst, loops, n, sizes=sizes, order=order, max_span=max(sizes) + 8)


# ------------------------------------------------------------------------------------------------ cases
# (heads, ch, head_pitch, ell) of the per-edge kernels: 15 = 3 x 4 + 3 channels compact and at a pitch of 16; 25: eight lanes per head;
# 16: every lane full; 17: eight lanes, the last three without a channel; 3 and 1: one partly filled lane
SHAPES = [(3, 15, 0, False), (3, 15, 16, True), (2, 15, 16, True), (2, 25, 0, False), (1, 16, 0, True), (2, 17, 0, False),
          (4, 3, 0, False), (1, 1, 0, False)]
PS = [0.1, 0.5]
# (pair_key, recomputed backward): the position key cannot be found from the source side, so it has the stored backward only
KEYS = [(False, False), (True, False), (True, True)]
KEY_IDS = ["position-stored", "pair-stored", "pair-recomputed"]
COUNTER_SHAPE, COUNTER_P = (3, 15, 16, True), 0.1      # the case that also runs with the step counter installed, under every key

# (heads, ch, p, loops_p) of the dense-block forms, and the seed of each one's graph
DENSE_CASES = [(2, 15, 0.1, 0.3), (3, 15, 0.5, 0.6), (2, 13, 0.1, 1.0)]


def dense_graph_seed(heads):
    return 11 + heads


@functools.lru_cache(maxsize=None)
def host_mask(pair_key, heads, p, counter=None):
    """(entries, keep) of ``graph(pair_key)`` in its host order."""
    in_ptr, in_src, loops, e = graph(pair_key).host_csr()
    return Entries(in_ptr, in_src, loops, e), mask(in_ptr, in_src, loops, e, heads, p, DROP_SEED, counter, pair_key)


def mask_cases():
    """Every (pair_key, heads, p, counter) a per-edge case of test_gpu_attention_dropout.py draws a mask for."""
    seen = []
    for heads, _, _, _ in SHAPES:
        for p in PS:
            for pair_key in (False, True):
                seen.append((pair_key, heads, p, None))
    for pair_key in (False, True):
        seen.append((pair_key, COUNTER_SHAPE[0], COUNTER_P, COUNTER))
    return sorted(set(seen), key=str)
