"""The attention kernels with fewer than three channels in all (H C < 3): a lane's 16-byte key / value segment then ends past the
qkvs ROW -- in the next row, or, for the last row, past the buffer.  Nothing that lies there may reach a result: the memory after a
tensor belongs to the allocator and holds whatever was freed there (the int32 -1 of a leaf record reads as a NaN, and 0 * NaN is a
NaN).  The rows are laid out at the head of a longer buffer whose tail is set, so the floats after the last row are known: forward,
inference and backward must give the same bits for a tail of zeros, of NaNs and of infinities, and no NaN."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("heads,ch", [(1, 1), (2, 1), (1, 2)])
def test_nothing_after_a_row_reaches_the_results(heads, ch):
    from blackwater.native import ops
    from blackwater.native.structure import GraphStructure

    rng = np.random.RandomState(10 * heads + ch)
    n, hc = 67, heads * ch
    deg = rng.choice([0, 1, 2, 3, 5, 9], size=n)
    dst = np.repeat(np.arange(n), deg)
    src = rng.randint(0, n, size=dst.shape[0])
    src[::3] = n - 1                                                    # the last row is a source of many entries
    src = np.where(src == dst, (src + 1) % n, src)
    loops = rng.randint(0, 3, size=n)
    loops[n - 1] = 1                                                    # ... and its own, through its self entry
    ei = np.concatenate([np.stack([src, dst]), np.repeat(np.stack([np.arange(n)] * 2), loops, axis=1)], axis=1)
    s = GraphStructure.from_edge_index(torch.from_numpy(ei).to(DEV), n)
    g = torch.Generator().manual_seed(ch)
    rows = torch.randn(n, 4 * hc, generator=g).to(DEV)
    gout = torch.randn(n, hc, generator=g).to(DEV)

    def run(tail):
        buf = torch.zeros(n * 4 * hc + 16, device=DEV)
        buf[n * 4 * hc:] = tail
        buf[:n * 4 * hc] = rows.reshape(-1)
        qkvs = buf[:n * 4 * hc].view(n, 4 * hc)
        out, attn, m, den = ops.transformer_attention_train(qkvs, s.in_ptr, s.in_src, s.loops, s.edge_count(), heads, ch)
        gq = ops.transformer_attention_bwd(qkvs, gout, attn, m, den, s, s.edge_count(), heads, ch)
        inf = ops.transformer_attention(qkvs, s.in_ptr, s.in_src, s.loops, heads, ch)
        return out, inf, gq

    want = run(0.0)
    assert all(bool(torch.isfinite(t).all()) for t in want)
    for tail in (float("nan"), float("inf")):
        got = run(tail)
        for name, a, b in zip(("out", "inference", "gradient"), want, got):
            assert bool(torch.isfinite(b).all()), f"{name}: what lies after the last row reached the result"
            assert torch.equal(a, b), name
