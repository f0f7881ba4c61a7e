"""k_colsum_reduce (csrc/bias_grad_kernels.hip): G fp32 partial rows of N
columns -> bf16 column sums, against the fp64 sum with the bound derived in
colsum_bounds.py for the kernel's summation tree.  Partials of mixed sign
over a wide magnitude range; repeats bit-equal; guards around the outputs
untouched; one and three outputs (the add+LayerNorm layout)."""
import pytest
import torch

from colsum_bounds import colsum_check, reduce_adds
from test_gpu_fused_attn import CANARY_BF16, GUARD, _guarded

pytestmark = pytest.mark.gpu

GS = [1, 2, 55, 512, 1024]
NS = [64, 192, 1536, 2304]


def _partials(G, N):
    g = torch.Generator(device="cuda").manual_seed(100 * G + N)
    mant = torch.randn(G, N, device="cuda", generator=g)
    expo = torch.randint(-12, 13, (G, N), device="cuda", generator=g)
    return torch.ldexp(mant, expo).float().contiguous()


def _run(part, G, N, nout):
    from sharedtensor_amd import _core
    seg = N // nout
    bufs, outs = zip(*(_guarded((seg,), torch.bfloat16, CANARY_BF16)
                       for _ in range(nout)))
    ptrs = [o.data_ptr() for o in outs] + [0] * (3 - nout)
    _core.colsum_reduce(part.data_ptr(), G, N, seg, *ptrs,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    guard = torch.full((GUARD,), CANARY_BF16, dtype=torch.bfloat16,
                       device="cuda")
    for b in bufs:
        assert torch.equal(b[:GUARD], guard) and torch.equal(b[-GUARD:], guard)
    return torch.cat(outs)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("G", GS)
def test_colsum_reduce(G, N):
    part = _partials(G, N)
    keep = part.clone()
    for nout in (1, 3) if N % 24 == 0 else (1,):
        got = _run(part, G, N, nout)
        worst = colsum_check(got, part, reduce_adds(G),
                             f"colsum_reduce G={G} N={N} nout={nout}")
        print(f"MAXERR op=colsum_reduce G={G} N={N} nout={nout} "
              f"{worst:.4g} of-bound")
        assert torch.equal(got, _run(part, G, N, nout)), "repeat differs"
    assert torch.equal(part, keep), "the partials were written"


def test_null_output_is_skipped():
    from sharedtensor_amd import _core
    G, N = 7, 192
    part = _partials(G, N)
    buf, out = _guarded((64,), torch.bfloat16, CANARY_BF16)
    _core.colsum_reduce(part.data_ptr(), G, N, 64, 0, out.data_ptr(), 0,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    colsum_check(out, part[:, 64:128], reduce_adds(G), "middle output")


def test_bad_shapes_raise():
    from sharedtensor_amd import _core
    part = _partials(2, 64)
    out = torch.empty(64, dtype=torch.bfloat16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for G, N, seg in ((0, 64, 64), (2, 62, 62), (2, 64, 16)):
        with pytest.raises(RuntimeError):
            _core.colsum_reduce(part.data_ptr(), G, N, seg, out.data_ptr(),
                                0, 0, s)
    with pytest.raises(RuntimeError):
        _core.colsum_reduce(part.data_ptr() + 4, 2, 64, 64, out.data_ptr(),
                            0, 0, s)
