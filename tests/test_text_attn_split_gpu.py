"""pnc_attn_text_split_f16 (include/panacea_hip.h section 6c) on the MI355X against the float64 reference and the derived bound of
tests/text_attn_split_ref64.py (tests/test_text_attn_split.py shows on the CPU that eight wrong kernels fall outside that bound, by a
factor of at least 2, on these very operands and shapes).

The kernel works on 16-query x 16-key tiles and visits the key tiles up to the diagonal and up to the last valid key: the shapes
ref64.SHAPES cover every edge of both, a one-key row, the product's (80, 77) and the largest accepted (96, 96).  Every run is made
twice, on POISONED operands (key and value rows >= kv_valid NaN, row padding NaN, buffers that end right behind their last named
element) and on clean ones (zeros there): the outputs must be finite and equal bit for bit; the unnamed elements of o and o_lo hold a
bit pattern of their own and are compared before and after."""
import ctypes

import pytest
import torch

import text_attn_split_ref64 as ref64
from helpers import measured
from panacea_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _operands(planes, kv_valid, layout, fill):
    """-> (the nine arguments in front of `o` on the device, the same on the host).  `fill` goes to the key and value rows >= kv_valid
    and to the row padding.  layout "qkv": column blocks of ONE [M, 3W] buffer, ld = 3W; "planes": separate planes, ld = W + 8, each
    buffer ending behind its last named element."""
    pl = {n: t.clone() for n, t in planes.items()}
    for n in ("k", "k_lo", "v", "v_lo"):
        pl[n][:, kv_valid:] = fill
    W = pl["q"].shape[-1]
    if layout == "qkv":
        (_, (qh, kh, vh)), (_, (ql, kl, vl)) = ref64.qkv_buffer(pl, ""), ref64.qkv_buffer(pl, "_lo")
        host = (qh, ql, 3 * W, kh, kl, 3 * W, vh, vl, 3 * W)
        dh, dl = qh.to(DEV), ql.to(DEV)
        return (dh, dl, 3 * W, dh[W:], dl[W:], 3 * W, dh[2 * W:], dl[2 * W:], 3 * W), host
    ld = W + 8
    host = tuple(x for n in ("q", "k", "v") for x in (ref64.embed(pl[n], ld, fill), ref64.embed(pl[n + "_lo"], ld, fill), ld))
    return tuple(x.to(DEV) if torch.is_tensor(x) else x for x in host), host


def _launch(ops, ldo, *, groups, heads, Lp, kv_valid, scale):
    """-> (o, o_lo) as fp16 [groups, Lp, W] on the host; everything but the named elements of either plane must keep its bits"""
    W = 64 * heads
    n = (groups * Lp - 1) * ldo + W
    seed = (torch.arange(n, dtype=torch.int64) * 40503 % 65536 - 32768).to(torch.int16)          # NaN, Inf and finite patterns alike
    o, o_lo = seed.clone().to(DEV).view(torch.float16), seed.clone().to(DEV).view(torch.float16)
    hip.attn_text_split(*ops, o, o_lo, ldo, groups=groups, heads=heads, Lp=Lp, kv_valid=kv_valid, scale=scale)
    torch.cuda.synchronize()
    named = ref64.named_mask(ldo, F=groups, N=Lp, C=W)
    out = []
    for name, t in (("o", o), ("o_lo", o_lo)):
        t = t.cpu()
        assert torch.equal(t.view(torch.int16)[~named], seed[~named]), f"unnamed elements of {name} were written"
        out.append(t[named].reshape(groups, Lp, W))
    return out


def _check(tag, planes, scale, *, groups, heads, Lp, kv_valid, layout, ldo):
    geo = dict(groups=groups, heads=heads, Lp=Lp, kv_valid=kv_valid, scale=scale)
    ops, host = _operands(planes, kv_valid, layout, float("nan"))
    ref, bnd = ref64.attn_text_split(*host, **geo)
    o, o_lo = _launch(ops, ldo, **geo)
    got = ref64.value(o, o_lo)
    finite = bool(torch.isfinite(got).all())
    err, over = ref64.excess(got, ref, bnd) if finite else (float("nan"), float("nan"))
    frac = ((got - ref).abs() / bnd).max().item() if finite else float("nan")
    print(f"{tag}: attn_text_split_kernel vs float64 max|err| {err:.3e}, {frac:.3f} of the bound (|ref| max {ref.abs().max().item():.2f})")
    measured("text_attn_split " + tag.replace(" ", "_"), kernel="attn_text_split_kernel", max_err=err, of_bound=frac)
    assert finite, f"{tag}: non-finite output in rows < Lp on poisoned buffers"
    assert over <= 0, f"{tag}: max|err| {err:.4e} is {frac:.2f} times the derived bound"
    o2, o2_lo = _launch(ops, ldo, **geo)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(o_lo.view(torch.int16), o2_lo.view(torch.int16)), f"{tag}: two runs differ"
    clean, _ = _operands(planes, kv_valid, layout, 0.0)
    o3, o3_lo = _launch(clean, ldo, **geo)
    assert torch.equal(o.view(torch.int16), o3.view(torch.int16)) and torch.equal(o_lo.view(torch.int16), o3_lo.view(torch.int16)), \
        f"{tag}: the poison behind kv_valid / in the padding reached the output"
    return o


# ------------------------------------------------------------------------------------------ the kernel against float64, poisoned
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("heads", [1, 2, 16])
@pytest.mark.parametrize("Lp,kv", ref64.SHAPES)
def test_kernel_vs_float64_on_poisoned_buffers(Lp, kv, heads, groups):
    planes, scale = ref64.case("unit", groups=groups, heads=heads, Lp=Lp)
    W = 64 * heads
    for layout in ("qkv", "planes"):
        for ldo in (W, W + 8):
            _check(f"Lp{Lp} kv{kv} h{heads} g{groups} {layout} ldo{ldo}", planes, scale, groups=groups, heads=heads, Lp=Lp, kv_valid=kv,
                   layout=layout, ldo=ldo)


# ------------------------------------------------------------------------------------------ exact data
def test_one_hot_rows_return_v_bit_for_bit():
    """q_i = 48 e_i, k_j = 8 e_j, scale = 1/8: query i sees 48 at its own key and 0 elsewhere, so every other probability is e^-48, 0 in
    both planes of P, and the row sum is 1 in fp32.  v holds distinct integers of [-2048, 2047] (exact in fp16), all lo planes are 0:
    o must be v bit for bit and o_lo must be 0.  A permuted fragment map cannot pass this."""
    groups, heads, Lp = 2, 2, 64
    W = 64 * heads
    eye = torch.eye(64, dtype=torch.float16)
    q = (48 * eye)[None, :, None, :].expand(groups, Lp, heads, 64).reshape(groups, Lp, W)
    k = (8 * eye)[None, :, None, :].expand(groups, Lp, heads, 64).reshape(groups, Lp, W)
    g, i, c = torch.meshgrid(torch.arange(groups), torch.arange(Lp), torch.arange(W), indexing="ij")
    v = (((i * 64 + c % 64) * 7 + 3 * (c // 64) + 5 * g) % 4096 - 2048).to(torch.float16)
    for h in range(heads):
        assert v[0, :, 64 * h: 64 * h + 64].unique().numel() == 64 * 64
    zero = torch.zeros_like(v)
    planes = dict(q=q.contiguous(), q_lo=zero, k=k.contiguous(), k_lo=zero, v=v, v_lo=zero)
    for layout in ("qkv", "planes"):
        ops, _ = _operands(planes, Lp, layout, float("nan"))
        o, o_lo = _launch(ops, W + 8, groups=groups, heads=heads, Lp=Lp, kv_valid=Lp, scale=0.125)
        assert torch.equal(o.view(torch.int16), v.view(torch.int16)), layout
        assert torch.equal(o_lo.view(torch.int16), zero.view(torch.int16)), layout


# ------------------------------------------------------------------------------------------ zero lo planes: the single-plane kernel
def test_zero_lo_planes_within_one_fp16_ulp_of_the_single_plane_causal_launch():
    """All lo planes zero: o against hip.attn_views(..., causal=True) — the tower's `fast` launch — on the same data, within ONE fp16
    ulp per element.  v lies in [1, 2): every output is a convex combination of values of one binade, so one ulp is 2^-10 for every
    element, and the single-plane kernel's fp16 P (relative 2^-11 per probability, against deviations |v_j - o| < 1) stays below it."""
    B, H, L, Lp = 2, 16, 77, 80
    W = 64 * H
    g = torch.Generator().manual_seed(11)
    q, k = (torch.randn(B, Lp, W, generator=g).half() for _ in range(2))
    v = (1.0 + torch.rand(B, Lp, W, generator=g) * (1.0 - 2.0 ** -10)).half()
    assert 1.0 <= v.float().min().item() and v.float().max().item() < 2.0
    zero = torch.zeros_like(v)
    planes = dict(q=q, q_lo=zero, k=k, k_lo=zero, v=v, v_lo=zero)
    scale = 64 ** -0.5
    ops, _ = _operands(planes, L, "qkv", float("nan"))
    o, o_lo = _launch(ops, W, groups=B, heads=H, Lp=Lp, kv_valid=L, scale=scale)
    qk = torch.cat([q.reshape(B * Lp, W), k.reshape(B * Lp, W)], dim=1).contiguous().to(DEV)
    vt = v.clone()
    vt[:, L:] = 0
    vt = vt.transpose(1, 2).contiguous().to(DEV)                 # [B, W, Lp], zero behind the last real token (the tower's layout)
    o1 = torch.zeros((B * Lp, W), device=DEV, dtype=torch.float16)
    hip.attn_views(qk, 2 * W, qk.view(-1)[W:], 2 * W, vt, Lp, W * Lp, o1, W, groups=B, heads=H, H=1, W=Lp, views=1, kvH=1, kvW=Lp,
                   kv_views=1, kv_rows_per_group=Lp, q_per_kv=1, kv_valid=L, segs=[[0]], scale=scale, causal=True)
    torch.cuda.synchronize()
    o1 = o1.cpu().reshape(B, Lp, W)
    d = (o.float() - o1.float()).abs()
    print(f"zero lo planes: split hi vs attn_views(causal) max|diff| {d.max().item():.3e} (one ulp: {2.0 ** -10:.3e}); "
          f"{int((d > 0).sum())} of {d.numel()} elements differ")
    measured("text_attn_split zero_lo", max_diff=d.max().item(), ulp=2.0 ** -10)
    assert torch.isfinite(o.float()).all() and 1.0 <= o.float().min().item() and o.float().max().item() < 2.0
    assert d.max().item() <= 2.0 ** -10


# ------------------------------------------------------------------------------------------ the refusal table, one case per rule
def test_refusals_leave_o_unchanged():
    groups, heads, Lp, kv = 1, 2, 16, 9
    W = 64 * heads
    planes, scale = ref64.case("unit", groups=groups, heads=heads, Lp=Lp)
    t = {n: p.reshape(groups * Lp, W).to(DEV) for n, p in planes.items()}
    o = torch.full((groups * Lp + 1, W + 8), 3.0, device=DEV, dtype=torch.float16)
    o_lo = torch.full((groups * Lp + 1, W + 8), 5.0, device=DEV, dtype=torch.float16)
    lib = hip.load()
    P = ctypes.c_void_p

    def call(groups=groups, heads=heads, Lp=Lp, kv_valid=kv, ldq=W, ldk=W, ldv=W, ldo=W + 8, **over):
        p = {n: t[n].data_ptr() for n in t}
        p.update(o=o.data_ptr(), o_lo=o_lo.data_ptr())
        p.update(over)
        a = {n: (None if x is None else P(x)) for n, x in p.items()}
        return lib.pnc_attn_text_split_f16(a["q"], a["q_lo"], ldq, a["k"], a["k_lo"], ldk, a["v"], a["v_lo"], ldv, a["o"], a["o_lo"], ldo,
                                           groups, heads, Lp, kv_valid, ctypes.c_float(scale), None)

    big = 2 ** 21
    rules = [("null pointer", dict(k_lo=None), -1), ("groups < 1", dict(groups=0), -1), ("heads < 1", dict(heads=0), -1),
             ("groups * heads >= 2^31", dict(groups=2 ** 16, heads=2 ** 15, ldq=big, ldk=big, ldv=big, ldo=big), -1),
             ("Lp % 8", dict(Lp=12, kv_valid=9), -1), ("Lp < 8", dict(Lp=0, kv_valid=0), -1), ("Lp > 96", dict(Lp=104), -1),
             ("kv_valid < 1", dict(kv_valid=0), -1), ("kv_valid > Lp", dict(kv_valid=Lp + 1), -1),
             ("leading dimension below 64 heads", dict(ldv=W - 8), -1),
             ("a range ahead of a leading dimension", dict(kv_valid=0, ldo=W + 4), -1),
             ("leading dimension no multiple of 8", dict(ldo=W + 4), -2),
             ("a leading dimension ahead of a pointer", dict(ldk=W + 2, o=o.data_ptr() + 8), -2),
             ("pointer off 16 bytes", dict(o_lo=o_lo.data_ptr() + 8), -2)]
    for what, kw, code in rules:
        assert call(**kw) == code, what
        torch.cuda.synchronize()
        assert bool((o == 3.0).all()) and bool((o_lo == 5.0).all()), f"{what}: something was launched"
    assert call() == 0                                            # PNC_OK: the call they all vary is a valid one
    torch.cuda.synchronize()
    n = groups * Lp
    assert bool((o[:n, :W] != 3.0).any()) and bool((o[:, W:] == 3.0).all()) and bool((o[n:] == 3.0).all())
    assert bool((o_lo[:n, :W] != 5.0).any()) and bool((o_lo[:, W:] == 5.0).all()) and bool((o_lo[n:] == 5.0).all())
