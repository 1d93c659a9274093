"""What the attention and norm entry points return for bad arguments, on the CPU: a table of (entry point, arguments, expected
return code), one row per rejecting `return` of their argument checks, each fault alone on otherwise valid arguments.  A rejected
call returns before it launches, and only rejecting rows call a launching entry point: no device is needed and the pointers (into a
host buffer) are never followed.  The expected codes are what the library returned before the host layers of attn.hip,
attn_split.hip and norm.hip were restructured (commit cd4909f, loaded through PANACEA_HIP_LIB): this file passes on that library
unchanged.

pnc_attn_uses_text_kernel is pure host code, so its rows also accept: the text geometry under PNC_OPT_ATTN_VARIANT 0 and 43, and
each way out of attn_text_dispatch.

No row: the second `return PNC_EINVAL` of pnc_concat_add_stats (more than 3 float4 vectors per lane after slicing) cannot be reached —
C is a multiple of 64 up to 3072 there, which always slices down to 3."""
import ctypes as C

import pytest

from panacea_amd import hip

EINVAL, EALIGN, EABI = -1, -2, -3
_BUF = (C.c_char * 256)()
A16 = (C.addressof(_BUF) + 15) & ~15          # 16-byte aligned
A8, A2, NULL = A16 + 8, A16 + 2, None         # 8- but not 16-byte aligned; 2-byte aligned; no pointer


def _attn(**over):
    """a valid PncAttnParams (2 views of 32 columns, 8 rows, keys of the same grid, one segment per view), then `over`"""
    f = dict(q=A16, ldq=64, k=A16, ldk=64, vt=A16, ldvt=256, vt_gstride=64 * 256, o=A16, ldo=64, groups=1, heads=1, H=8, W=64, views=2,
             kvH=8, kvW=64, kv_views=2, kv_rows_per_group=512, q_per_kv=1, kv_valid=256, nseg=[1, 1], seg=[[0], [1]], scale=0.125, causal=0,
             k_halo=[NULL, NULL], vt_halo=[NULL, NULL])
    f.update(over)
    p = hip.AttnParams()
    for name, val in f.items():
        if name == "seg":
            for v, row in enumerate(val):
                for j, u in enumerate(row):
                    p.seg[v][j] = u
        elif isinstance(val, list):
            for i, u in enumerate(val):
                getattr(p, name)[i] = u
        else:
            setattr(p, name, val)
    return p


def _split(struct_bytes=None, lo=None, **over):
    sp = hip.AttnSplitParams()
    sp.struct_bytes = C.sizeof(hip.AttnSplitParams) if struct_bytes is None else struct_bytes
    sp.a = _attn(**over)
    sp.q_lo = sp.k_lo = sp.v_lo = sp.o_lo = A16
    for name, val in (lo or {}).items():
        setattr(sp, name, val)
    return sp


def _args(base, **over):
    """positional arguments of an entry point from its ordered `base` dict, then `over`; the stream (NULL) goes last"""
    assert set(over) <= set(base), over
    return tuple({**base, **over}.values()) + (None,)


TEMPORAL = dict(q=A16, ldq=64, k=A16, ldk=64, v=A16, ldv=64, o=A16, ldo=64, B=1, T=4, Npix=3, heads=1, scale=0.125)
TEMPORAL_SPLIT = dict(q=A16, q_lo=A16, ldq=64, k=A16, k_lo=A16, ldk=64, v=A16, v_lo=A16, ldv=64, o=A16, o_lo=A16, ldo=64, B=1, T=4, Npix=3,
                      heads=1, scale=0.125)
GN_STATS = dict(x=A16, ldx=64, F=1, Npix=5, C=64, ppc=4, partial=A16)
CONCAT = dict(a=A16, C1=32, s=A16, c=A16, C2=32, F=1, Npix=5, ppc=4, out32=A16, out16=A16, out16_lo=A16, lo_fmt=hip.LO_F16, partial=A16)
GN_APPLY = dict(x=A16, ldx=64, F=1, Npix=5, C=64, ppc=4, partial=A16, gamma=A16, beta=A16, eps=1e-5, silu=1, y16=A16, ldy=64, y16_lo=A16,
                lo_fmt=hip.LO_F16, n_records=0)
GN_COMBINE = dict(parts_in=A16, parts=2, F=1, nchunk=2, out=A16)
GN_T_SILU = dict(x=A16, B=1, T=4, Npix=3, C=64, gamma=A16, beta=A16, eps=1e-5, y16=A16, y16_lo=A16, lo_fmt=hip.LO_F16)
GN_T_PART = dict(x=A16, B=1, T=4, Npix=3, C=64, gamma=A16, beta=A16, eps=1e-5, stats=A16, mode=2, T_total=4, y16=A16, y16_lo=A16,
                 lo_fmt=hip.LO_F16, t_pad=0)
LAYERNORM = dict(x=A16, ldx=64, M=3, C=64, gamma=A16, beta=A16, eps=1e-5, y16=A16, ldy=64, y16_lo=A16)

ROWS = []


def _row(entry, tag, args, want):
    ROWS.append(pytest.param(entry, args, want, id=f"{entry[4:]}-{tag}"))


def _each(entry, base, want, **faults):
    """one row per (field, bad value): `base` with that field alone replaced"""
    for name, bad in faults.items():
        for b in bad if isinstance(bad, (list, tuple)) else [bad]:
            _row(entry, f"{name}={'NULL' if b is None else b - A16 if isinstance(b, int) and b >= A16 else b}", _args(base, **{name: b}), want)


# ---- pnc_attn_views_f16 (attn_views_check) -----------------------------------------------------------------------------------
V = "pnc_attn_views_f16"
_row(V, "params=NULL", (None, None), EINVAL)
for tag, over, want in [
        ("q=NULL", dict(q=NULL), EINVAL), ("k=NULL", dict(k=NULL), EINVAL), ("vt=NULL", dict(vt=NULL), EINVAL), ("o=NULL", dict(o=NULL), EINVAL),
        ("views=0", dict(views=0), EINVAL), ("views=9", dict(views=9), EINVAL), ("kv_views=0", dict(kv_views=0), EINVAL),
        ("kv_views=9", dict(kv_views=9), EINVAL), ("W%views", dict(W=65), EINVAL), ("kvW%kv_views", dict(kvW=65), EINVAL),
        ("ldq%8", dict(ldq=68), EALIGN), ("ldk%8", dict(ldk=68), EALIGN), ("ldo%4", dict(ldo=66), EALIGN),
        ("q&15", dict(q=A8), EALIGN), ("k&15", dict(k=A8), EALIGN), ("vt&15", dict(vt=A8), EALIGN), ("o&7", dict(o=A2), EALIGN),
        ("q_per_kv=0", dict(q_per_kv=0), EINVAL), ("groups=0", dict(groups=0), EINVAL), ("heads=0", dict(heads=0), EINVAL),
        ("kv_valid=0", dict(kv_valid=0), EINVAL), ("kv_valid>view", dict(kv_valid=257), EINVAL), ("causal=2", dict(causal=2), EINVAL),
        ("nseg=0", dict(nseg=[1, 0]), EINVAL), ("nseg=3", dict(nseg=[3, 1]), EINVAL),
        ("halo-left-missing", dict(seg=[[-1], [1]]), EINVAL), ("halo-right-missing", dict(seg=[[0], [2]]), EINVAL),
        ("halo-vt-missing", dict(seg=[[-1], [1]], k_halo=[A16, NULL]), EINVAL),
        ("halo&15", dict(seg=[[-1], [1]], k_halo=[A16, NULL], vt_halo=[A8, NULL]), EALIGN),
        ("seg=-2", dict(seg=[[-2], [1]]), EINVAL), ("seg>kv_views", dict(seg=[[0], [3]]), EINVAL)]:
    _row(V, tag, (_attn(**over), None), want)
# two faults at once, where the codes differ: this entry point looks at the view counts, then at alignment, then at the other counts,
# then walks the views (so a misaligned halo of view 0 is met before the segment count of view 1)
for tag, over, want in [
        ("order:views,ldq", dict(W=65, ldq=68), EINVAL), ("order:ldq,heads", dict(ldq=68, heads=0), EALIGN), ("order:q,kv_valid", dict(q=A8, kv_valid=0), EALIGN),
        ("order:o,nseg", dict(o=A2, nseg=[0, 1]), EALIGN), ("order:halo,nseg", dict(seg=[[-1], [1]], k_halo=[A16, NULL], vt_halo=[A8, NULL], nseg=[1, 0]), EALIGN)]:
    _row(V, tag, (_attn(**over), None), want)

# ---- pnc_attn_views_split_f16 --------------------------------------------------------------------------------------------------
S = "pnc_attn_views_split_f16"
_row(S, "params=NULL", (None, None), EINVAL)
_row(S, "struct_bytes", (_split(struct_bytes=C.sizeof(hip.AttnSplitParams) - 8), None), EABI)
for tag, lo, over, want in [
        ("q=NULL", None, dict(q=NULL), EINVAL), ("k=NULL", None, dict(k=NULL), EINVAL), ("v=NULL", None, dict(vt=NULL), EINVAL),
        ("o=NULL", None, dict(o=NULL), EINVAL), ("q_lo=NULL", dict(q_lo=NULL), {}, EINVAL), ("k_lo=NULL", dict(k_lo=NULL), {}, EINVAL),
        ("v_lo=NULL", dict(v_lo=NULL), {}, EINVAL), ("o_lo=NULL", dict(o_lo=NULL), {}, EINVAL),
        ("causal=1", None, dict(causal=1), EINVAL), ("k_halo", None, dict(k_halo=[NULL, A16]), EINVAL), ("vt_halo", None, dict(vt_halo=[A16, NULL]), EINVAL),
        ("views=0", None, dict(views=0), EINVAL), ("views=9", None, dict(views=9), EINVAL), ("kv_views=0", None, dict(kv_views=0), EINVAL),
        ("kv_views=9", None, dict(kv_views=9), EINVAL), ("W%views", None, dict(W=65), EINVAL), ("kvW%kv_views", None, dict(kvW=65), EINVAL),
        ("q_per_kv=0", None, dict(q_per_kv=0), EINVAL), ("groups=0", None, dict(groups=0), EINVAL), ("heads=0", None, dict(heads=0), EINVAL),
        ("H=0", None, dict(H=0), EINVAL), ("kvH=0", None, dict(kvH=0), EINVAL),
        ("kv_valid=0", None, dict(kv_valid=0), EINVAL), ("kv_valid>view", None, dict(kv_valid=257), EINVAL),
        ("kv_rows_per_group", None, dict(kv_rows_per_group=511), EINVAL),
        ("nseg=0", None, dict(nseg=[1, 0]), EINVAL), ("nseg=3", None, dict(nseg=[3, 1]), EINVAL),
        ("seg=-1", None, dict(seg=[[-1], [1]]), EINVAL), ("seg=kv_views", None, dict(seg=[[0], [2]]), EINVAL),
        ("ldq%4", None, dict(ldq=66), EALIGN), ("ldk%4", None, dict(ldk=66), EALIGN), ("ldv%4", None, dict(ldvt=66), EALIGN),
        ("ldo%4", None, dict(ldo=66), EALIGN), ("q&7", None, dict(q=A2), EALIGN), ("k&7", None, dict(k=A2), EALIGN),
        ("v&7", None, dict(vt=A2), EALIGN), ("o&7", None, dict(o=A2), EALIGN), ("q_lo&7", dict(q_lo=A2), {}, EALIGN),
        ("k_lo&7", dict(k_lo=A2), {}, EALIGN), ("v_lo&7", dict(v_lo=A2), {}, EALIGN), ("o_lo&7", dict(o_lo=A2), {}, EALIGN)]:
    _row(S, tag, (_split(lo=lo, **over), None), want)
# two faults at once: struct_bytes comes before the pointers, alignment after everything else
_row(S, "order:struct_bytes,q", (_split(struct_bytes=8, q=NULL), None), EABI)
_row(S, "order:nseg,ldq", (_split(nseg=[1, 3], ldq=66), None), EINVAL)

# ---- the temporal attentions ---------------------------------------------------------------------------------------------------
_each("pnc_attn_temporal_f16", TEMPORAL, EINVAL, q=NULL, k=NULL, v=NULL, o=NULL, T=[0, 17], B=0, Npix=0, heads=0)
_each("pnc_attn_temporal_f16", TEMPORAL, EALIGN, ldq=68, ldk=68, ldv=68, ldo=68, q=A8, k=A8, v=A8, o=A8)
_row("pnc_attn_temporal_f16", "wide-work>=2^31", _args(TEMPORAL, T=9, B=1 << 16, Npix=1 << 15), EINVAL)
_each("pnc_attn_temporal_split_f16", TEMPORAL_SPLIT, EINVAL, q=NULL, k=NULL, v=NULL, o=NULL, q_lo=NULL, k_lo=NULL, v_lo=NULL, o_lo=NULL,
      T=[0, 17], B=0, Npix=0, heads=0)
_each("pnc_attn_temporal_split_f16", TEMPORAL_SPLIT, EALIGN, ldq=66, ldk=66, ldv=66, ldo=66, q=A2, k=A2, v=A2, o=A2, q_lo=A2, k_lo=A2,
      v_lo=A2, o_lo=A2)

# ---- the norms -----------------------------------------------------------------------------------------------------------------
_each("pnc_groupnorm_stats", GN_STATS, EINVAL, x=NULL, partial=NULL, F=0, Npix=0, ppc=0, C=[96, 3136], ldx=66)
_each("pnc_groupnorm_stats", GN_STATS, EALIGN, x=A8)
_each("pnc_concat_add_stats", CONCAT, EINVAL, a=NULL, s=NULL, partial=NULL, F=0, Npix=0, ppc=0, C1=[30, 0, 64], C2=[30, 0], lo_fmt=2, out16=NULL)
_row("pnc_concat_add_stats", "no-output", _args(CONCAT, out32=NULL, out16=NULL, out16_lo=NULL), EINVAL)
_row("pnc_concat_add_stats", "C>3072", _args(CONCAT, C1=3072, C2=64), EINVAL)
_each("pnc_concat_add_stats", CONCAT, EALIGN, a=A8, s=A8, c=A8, out32=A8)
_each("pnc_groupnorm_apply", GN_APPLY, EINVAL, x=NULL, partial=NULL, gamma=NULL, beta=NULL, y16=NULL, F=0, Npix=0, ppc=0, n_records=-1,
      lo_fmt=2, C=[96, 3136], ldx=66, ldy=66)
_each("pnc_groupnorm_apply", GN_APPLY, EALIGN, x=A8, y16=A2, y16_lo=A2)
_each("pnc_groupnorm_combine", GN_COMBINE, EINVAL, parts_in=NULL, out=NULL, parts=0, F=0, nchunk=0)
_each("pnc_groupnorm_temporal_silu", GN_T_SILU, EINVAL, x=NULL, gamma=NULL, beta=NULL, y16=NULL, B=0, Npix=0, lo_fmt=2, C=[96, 2112], T=[0, 17])
_each("pnc_groupnorm_temporal_silu", GN_T_SILU, EALIGN, x=A8, gamma=A8, beta=A8, y16=A2, y16_lo=A2)
_each("pnc_groupnorm_temporal_part", GN_T_PART, EINVAL, x=NULL, stats=NULL, B=0, Npix=0, mode=[0, 3], C=[96, 2112], T=[0, 17], T_total=3,
      t_pad=2, gamma=NULL, beta=NULL, y16=NULL, lo_fmt=2)
_each("pnc_groupnorm_temporal_part", GN_T_PART, EALIGN, x=A8, gamma=A8, beta=A8, y16=A2, y16_lo=A2, stats=A2)
_each("pnc_layernorm", LAYERNORM, EINVAL, x=NULL, gamma=NULL, beta=NULL, y16=NULL, M=0, C=[66, 3076, 0], ldx=66, ldy=66)
_each("pnc_layernorm", LAYERNORM, EALIGN, x=A8, gamma=A8, beta=A8, y16=A2, y16_lo=A2)


@pytest.mark.parametrize("entry,args,want", ROWS)
def test_rejected_before_any_launch(entry, args, want):
    assert want < 0                       # only rejecting rows reach a launching entry point
    args = tuple(C.byref(a) if isinstance(a, C.Structure) else a for a in args)
    assert getattr(hip.load(), entry)(*args) == want


def test_the_base_arguments_are_the_entry_points_own():
    """the ordered base dicts above have one value per parameter of their entry point (the stream is added by _args)"""
    for entry, base in (("pnc_attn_temporal_f16", TEMPORAL), ("pnc_attn_temporal_split_f16", TEMPORAL_SPLIT), ("pnc_groupnorm_stats", GN_STATS),
                        ("pnc_concat_add_stats", CONCAT), ("pnc_groupnorm_apply", GN_APPLY), ("pnc_groupnorm_combine", GN_COMBINE),
                        ("pnc_groupnorm_temporal_silu", GN_T_SILU), ("pnc_groupnorm_temporal_part", GN_T_PART), ("pnc_layernorm", LAYERNORM)):
        assert len(base) + 1 == len(hip._SIGNATURES[entry][1]), entry


# ---- pnc_attn_uses_text_kernel: the dispatch predicate, accepting and refusing ---------------------------------------------------
def _text(**over):
    """77 text keys in a buffer of 80 rows, one view, 64 x 32 queries and 5 heads: 16 query tiles x 1 head group"""
    f = dict(H=64, W=32, views=1, kvH=1, kvW=80, kv_views=1, kv_rows_per_group=80, kv_valid=77, heads=5, ldq=320, ldk=320, ldo=320, ldvt=80,
             vt_gstride=320 * 80, nseg=[1], seg=[[0]])
    f.update(over)
    return _attn(**f)


SMALL = dict(H=8, W=32)         # 2 query tiles x 1 head group: fewer than 16 work items
TEXT_ROWS = [("text", {}, 0, None, 1), ("text", {}, 43, None, 1),
             ("causal", dict(causal=1), 43, None, 0), ("kv_valid=64", dict(kv_valid=64), 43, None, 0),
             ("77-row-buffer", dict(kvW=77, kv_rows_per_group=77), 43, None, 0), ("ldvt%8", dict(ldvt=84), 43, None, 0),
             ("small-unforced", SMALL, 0, None, 0), ("small-forced", SMALL, 43, None, 1),
             ("views-kernel-forced", {}, 42, None, 0), ("dma|4", {}, 43, 4, 0), ("bad-arguments", dict(heads=0), 43, None, 0)]


@pytest.mark.parametrize("over,variant,dma_bits,want", [pytest.param(*r[1:], id=f"{r[0]}-variant{r[2]}") for r in TEXT_ROWS])
def test_attn_uses_text_kernel(over, variant, dma_bits, want):
    lib = hip.load()
    prev_v = lib.pnc_set_option(hip.OPT_ATTN_VARIANT, variant)
    prev_d = lib.pnc_set_option(hip.OPT_ATTN_DMA, 0)
    lib.pnc_set_option(hip.OPT_ATTN_DMA, prev_d | (dma_bits or 0))
    try:
        assert lib.pnc_attn_uses_text_kernel(C.byref(_text(**over))) == want
    finally:
        lib.pnc_set_option(hip.OPT_ATTN_DMA, prev_d)
        lib.pnc_set_option(hip.OPT_ATTN_VARIANT, prev_v)
