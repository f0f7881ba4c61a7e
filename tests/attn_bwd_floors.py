"""fp64 reference and fp32 floors of the attention backward, shared by
tests/test_gpu_fused_attn_bwd.py and tests/test_fused_attn_bwd_cpu.py."""
import torch

EPS32 = 2.0 ** -24


def reference(q, k, v, dout, scale):
    """Plain softmax attention and its autograd in fp64.  (B, H, T, 64) in,
    dict of out, P, dq, dk, dv."""
    q, k, v = (t.detach().double().requires_grad_() for t in (q, k, v))
    T = q.shape[2]
    vis = torch.ones(T, T, device=q.device, dtype=torch.bool).tril()
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = p @ v
    out.backward(dout.double())
    return dict(out=out.detach(), P=p.detach(), dq=q.grad, dk=k.grad,
                dv=v.grad)


def floors(ref, q, k, v, dout, scale):
    """Element-wise floors of dq, dk, dv: what the fp32 operations alone can
    cost (the docstring of test_gpu_fused_attn_bwd.py derives the counts)."""
    q, k, v, do = (t.double().abs() for t in (q, k, v, dout))
    T = q.shape[2]
    a = ref["P"] * (do @ v.transpose(-1, -2)
                    + (do * ref["out"].abs()).sum(-1, keepdim=True))
    f_ds = a * (132 * EPS32 + 2.0 ** -20)
    return dict(dq=scale * (f_ds @ k),
                dk=scale * (f_ds.transpose(-1, -2) @ q),
                dv=(ref["P"].transpose(-1, -2) @ do)
                * ((T + 64) * EPS32 + 2.0 ** -20))
