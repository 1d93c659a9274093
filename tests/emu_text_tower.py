"""tests/emu.py plus the optional capability of the text tower's split policies: `attn_text_split`, a float64 evaluation of the
formulae of include/panacea_hip.h section 6c (CPU tensors only).  Everything else is delegated to `emu`; install an instance with
`engine.use_backend`.

    S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)                   lo.lo dropped
    query i attends key j  iff  j <= i and j < kv_valid
    P = softmax(scale * S) over the attended keys, carried as an fp16 pair Ph + 2^-11 Pl against the row maximum
    O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh), normalised by the row sum, written as o = fp16(O), o_lo = fp16((O - o) * 2^11)"""
import torch

import emu
import text_attn_split_ref64 as ref64

LO = 2.0 ** -11


class Backend:
    def __init__(self, with_split=True):
        self.split_calls = []
        if with_split:
            self.attn_text_split = self._attn_text_split

    def __getattr__(self, name):
        return getattr(emu, name)

    def _attn_text_split(self, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, groups, heads, Lp, kv_valid, scale):
        geo = dict(groups=groups, heads=heads, Lp=Lp)
        Qh, Ql = ref64.gather(q, ldq, rows=Lp, **geo), ref64.gather(q_lo, ldq, rows=Lp, **geo)
        Kh, Kl = ref64.gather(k, ldk, rows=kv_valid, **geo), ref64.gather(k_lo, ldk, rows=kv_valid, **geo)
        Vh, Vl = ref64.gather(v, ldv, rows=kv_valid, **geo), ref64.gather(v_lo, ldv, rows=kv_valid, **geo)
        att = ref64.attended(Lp, kv_valid)
        S = Qh @ Kh.transpose(2, 3) + LO * (Qh @ Kl.transpose(2, 3) + Ql @ Kh.transpose(2, 3))
        x = torch.where(att, scale * S, torch.full_like(S, -float("inf")))
        P = torch.exp(x - x.max(dim=-1, keepdim=True).values)          # exactly 0 at the keys a row does not attend
        Ph = P.float().half()
        Pl = ((P.float() - Ph.float()) * 2048.0).half()
        O = (Ph.double() @ Vh + LO * (Ph.double() @ Vl + Pl.double() @ Vh)) / P.sum(dim=-1, keepdim=True)
        hi, lo = ref64.split(O.permute(0, 2, 1, 3).reshape(groups * Lp, 64 * heads))
        idx = ((torch.arange(groups * Lp) * ldo)[:, None] + torch.arange(64 * heads)[None, :]).reshape(-1)
        for plane, val in ((o, hi), (o_lo, lo)):
            flat = plane.reshape(-1)
            assert flat.data_ptr() == plane.data_ptr(), "o / o_lo must be contiguous buffers"
            flat[idx] = val.reshape(-1)
        self.split_calls.append(dict(groups=groups, heads=heads, Lp=Lp, kv_valid=kv_valid, scale=scale, lds=(ldq, ldk, ldv, ldo)))
