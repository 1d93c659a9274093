"""Float64 single-head attention over the tokens of a frame, indexed from the words of include/panacea_hip.h section 6 alone.

Nothing here comes from tests/emu.py or from the kernel: every operand element is fetched from the FLAT storage of its buffer at
the address the header spells out, so a convention shared by a kernel and an emulation cannot hide in both.  Only the elements the
contract names are touched: a buffer may hold NaN everywhere else and may end right after its last named element.

    q / k row of (frame f, token i)     f*N + i, element c < C at               q[(f*N + i)*ldq + c],  k[(f*N + i)*ldk + c]
    V, channel-major per frame          channel c < C of key j < N at           vt[f*vt_fstride + c*ldvt + j]
    every token of a frame attends all N tokens of the same frame:              o = softmax(scale * q k^T) v

Operands are taken as they are (fp16 values); the result is float64."""
import torch


def _flat(t):
    return t.detach().cpu().reshape(-1)


def attn_frame(q, ldq, k, ldk, vt, ldvt, vt_fstride, *, F, N, C, scale, rows=None):
    """-> float64 [F, N, C], the rows of o with ldo = C; `rows` (a 1-D index tensor of query tokens): only those queries of every
    frame, [F, len(rows), C]"""
    qf, kf, vf = _flat(q), _flat(k), _flat(vt)
    c = torch.arange(C)
    j = torch.arange(N)
    qi = j if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    out = torch.empty((F, qi.numel(), C), dtype=torch.float64)
    for f in range(F):
        Q = qf[((f * N + qi) * ldq)[:, None] + c[None, :]].double()
        K = kf[((f * N + j) * ldk)[:, None] + c[None, :]].double()
        V = vf[f * vt_fstride + c[None, :] * ldvt + j[:, None]].double()          # [key, channel]
        S = (Q @ K.t()) * scale
        S = S - S.max(dim=-1, keepdim=True).values
        P = torch.exp(S)
        out[f] = (P / P.sum(dim=-1, keepdim=True)) @ V
    return out


def scatter_o(o, ldo, ref, *, F, N, C):
    """write ref [F, N, C], rounded to o's dtype, to the named elements of o: o[(f*N + i)*ldo + c] — everything else stays"""
    flat = o.reshape(-1)
    assert flat.data_ptr() == o.data_ptr(), "o must be a contiguous buffer"
    idx = ((torch.arange(F)[:, None] * N + torch.arange(N)[None, :]) * ldo)[:, :, None] + torch.arange(C)[None, None, :]
    flat[idx.reshape(-1)] = ref.reshape(-1).to(o.dtype)
