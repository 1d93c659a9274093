"""tests/emu.py plus the optional capability of the first stage's split policies: `attn_frame_split`, a float64 evaluation of the
formulae of include/panacea_hip.h section 6b (CPU tensors only).  Everything else is delegated to `emu`; install an instance with
`engine.use_backend`.

    S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)                   lo.lo dropped
    P = softmax(scale * S) per row, carried as an fp16 pair Ph + 2^-11 Pl against the row maximum
    O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh), normalised by the row sum, written as o = fp16(O), o_lo = fp16((O - o) * 2^11)"""
import torch

import emu
import frame_attn_split_ref64 as ref64

LO = 2.0 ** -11


class Backend:
    def __init__(self, with_split=True):
        self.split_calls = []
        if with_split:
            self.attn_frame_split = self._attn_frame_split

    def __getattr__(self, name):
        return getattr(emu, name)

    def _attn_frame_split(self, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, F, N, C, scale):
        geo = dict(F=F, N=N, C=C)
        Qh, Ql = ref64.gather(q, ldq, **geo), ref64.gather(q_lo, ldq, **geo)
        Kh, Kl = ref64.gather(k, ldk, **geo), ref64.gather(k_lo, ldk, **geo)
        Vh, Vl = ref64.gather(v, ldv, **geo), ref64.gather(v_lo, ldv, **geo)
        S = Qh @ Kh.transpose(1, 2) + LO * (Qh @ Kl.transpose(1, 2) + Ql @ Kh.transpose(1, 2))
        x = scale * S
        P = torch.exp(x - x.max(dim=-1, keepdim=True).values)
        Ph = P.float().half()
        Pl = ((P.float() - Ph.float()) * 2048.0).half()
        O = (Ph.double() @ Vh + LO * (Ph.double() @ Vl + Pl.double() @ Vh)) / P.sum(dim=-1, keepdim=True)
        hi, lo = ref64.split(O)
        idx = ((torch.arange(F * N) * ldo)[:, None] + torch.arange(C)[None, :]).reshape(-1)
        for plane, val in ((o, hi), (o_lo, lo)):
            flat = plane.reshape(-1)
            assert flat.data_ptr() == plane.data_ptr(), "o / o_lo must be contiguous buffers"
            flat[idx] = val.reshape(-1)
        self.split_calls.append(dict(F=F, N=N, C=C, scale=scale, lds=(ldq, ldk, ldv, ldo)))
