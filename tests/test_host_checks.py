"""What the attention, norm, misc and stats entry points return for bad arguments, on the CPU: a table of (entry point, arguments,
expected return code), one row per rejecting `return` of their argument checks, each fault alone on otherwise valid arguments.  A rejected
call returns before it launches, and only rejecting rows call a launching entry point: no device is needed and the pointers (into a
host buffer) are never followed.  The expected codes are what the library returned before the host layers of attn.hip,
attn_split.hip and norm.hip were restructured (commit cd4909f, loaded through PANACEA_HIP_LIB), and for the rows of misc.hip and
stats.hip what it returned when the Euler exit still had a kernel and a launch function of its own (commit da1a801): this file passes
on those libraries unchanged.

pnc_attn_uses_text_kernel is pure host code, so its rows also accept: the text geometry under PNC_OPT_ATTN_VARIANT 0 and 43, and
each way out of attn_text_dispatch.

No row: the second `return PNC_EINVAL` of pnc_concat_add_stats (more than 3 float4 vectors per lane after slicing) cannot be reached —
C is a multiple of 64 up to 3072 there, which always slices down to 3.  Nor can the PNC_EABI of the exit launch be reached through
pnc_cfg_euler_step[_skip]: they fill the parameter struct themselves.  The order among the checks of those two entries cannot be
seen (every one is PNC_EINVAL); where an entry point of misc.hip / stats.hip mixes codes, a two-fault row pins the order."""
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


# ---- the sampler exits (misc.hip) ------------------------------------------------------------------------------------------------
EULER = dict(eps_tok=A16, ld=8, T=2, Npix=5, C=4, cfg=1, scale=5.0, x=A16, c_out=A16, sigma=A16, sigma_next=A16, x_next=A16)
EULER_SKIP = dict(eps_tok=A16, ld=8, T=2, Npix=5, C=4, cfg=1, scale=5.0, x=A16, c_skip=A16, c_out=A16, sigma=A16, sigma_next=A16, x_next=A16)
for entry, base in (("pnc_cfg_euler_step", EULER), ("pnc_cfg_euler_step_skip", EULER_SKIP)):
    _each(entry, base, EINVAL, eps_tok=NULL, x=NULL, c_out=NULL, sigma=NULL, sigma_next=NULL, x_next=NULL, T=0, Npix=0, C=0, ld=3)
_each("pnc_cfg_euler_step_skip", EULER_SKIP, EINVAL, c_skip=NULL)


def _step(mode, struct_bytes=None, **over):
    """a PncSamplerStepParams with every operand any mode reads (n_hist = 3), then `over`; v / hist entries by index: v2=NULL"""
    p = hip.SamplerStepParams()
    p.struct_bytes = C.sizeof(hip.SamplerStepParams) if struct_bytes is None else struct_bytes
    p.mode, p.ld, p.T, p.Npix, p.C, p.cfg, p.scale, p.n_hist, p.s_noise = mode, 8, 2, 5, 4, 1, 5.0, 3, 1.0
    p.eps_tok = p.x = p.c_out = p.x0 = p.aux = p.noise = p.out = p.out_aux = A16
    for k in range(6):
        p.v[k] = A16
    for k in range(4):
        p.hist[k] = A16
    for name, val in over.items():
        if name[0] in "vh" and name[-1].isdigit():
            getattr(p, name.rstrip("0123456789"))[int(name[-1])] = val
        else:
            setattr(p, name, val)
    return p


# what each mode cannot do without: its operands and its per-frame vectors (DPM2M reads v[2..4] only next to a previous D)
STEP_NEEDS = {hip.SAMPLER_HEUN1: ("out_aux", "v0", "v1"), hip.SAMPLER_HEUN2: ("x0", "aux", "v0", "v1"),
              hip.SAMPLER_EULER_A: ("noise", "v0", "v1", "v2", "v3"), hip.SAMPLER_DPM2S_1: ("out_aux", "v0", "v1", "v2", "v3"),
              hip.SAMPLER_DPM2S_2: ("x0", "aux", "noise", "v0", "v1", "v2", "v3", "v4"),
              hip.SAMPLER_DPM2M: ("out_aux", "v0", "v1", "v2", "v3", "v4"), hip.SAMPLER_LMS: ("out_aux", "hist0", "hist1", "hist2", "v0", "v1", "v2", "v3", "v4")}
for entry, tail in (("pnc_cfg_sampler_step", (None,)), ("pnc_cfg_sampler_step_skip", (A16, None))):
    _row(entry, "params=NULL", (None,) + tail, EABI)
    _row(entry, "struct_bytes", (_step(0, struct_bytes=C.sizeof(hip.SamplerStepParams) - 8),) + tail, EABI)
    _row(entry, "struct_bytes=0", (_step(0, struct_bytes=0),) + tail, EABI)
    for tag, over in [("eps_tok=NULL", dict(eps_tok=NULL)), ("x=NULL", dict(x=NULL)), ("c_out=NULL", dict(c_out=NULL)), ("out=NULL", dict(out=NULL)),
                      ("T=0", dict(T=0)), ("Npix=0", dict(Npix=0)), ("C=0", dict(C=0)), ("ld<C", dict(ld=3))]:
        _row(entry, tag, (_step(hip.SAMPLER_HEUN2, **over),) + tail, EINVAL)
    for mode, needs in STEP_NEEDS.items():
        for name in needs:
            _row(entry, f"mode{mode}-{name}=NULL", (_step(mode, **{name: NULL}),) + tail, EINVAL)
    _row(entry, "mode5-first-step-v1=NULL", (_step(hip.SAMPLER_DPM2M, aux=NULL, v1=NULL),) + tail, EINVAL)
    for n_hist in (-1, 4):
        _row(entry, f"mode6-n_hist={n_hist}", (_step(hip.SAMPLER_LMS, n_hist=n_hist),) + tail, EINVAL)
    for mode in (-1, 7):                                           # 7: no public mode stands for "HEUN1 without out_aux"
        _row(entry, f"mode={mode}", (_step(mode),) + tail, EINVAL)
    _row(entry, "order:struct_bytes,eps_tok", (_step(0, struct_bytes=8, eps_tok=NULL),) + tail, EABI)
    _row(entry, "order:struct_bytes,mode", (_step(7, struct_bytes=8),) + tail, EABI)
_row("pnc_cfg_sampler_step_skip", "c_skip=NULL", (_step(hip.SAMPLER_HEUN2), None, None), EINVAL)
_row("pnc_cfg_sampler_step_skip", "order:struct_bytes,c_skip", (_step(0, struct_bytes=8), None, None), EABI)

# ---- the small-M linears ---------------------------------------------------------------------------------------------------------
SEGS = (C.c_int32 * 3)(0, 8, 16)
SEG_PTR = C.addressof(SEGS)


def _segs(*start):
    arr = (C.c_int32 * len(start))(*start)
    _segs.keep.append(arr)                 # the rows hold the address only
    return C.addressof(arr)


_segs.keep = []
SMALLM = dict(a=A16, lda=64, W=A16, bias=A16, out=A16, ldo=16, M=2, N=16, K=64, silu_in=0, silu_out=0)
SMALLM_SPLIT = dict(a=A16, lda=64, W=A16, W_lo=A16, bias=A16, out=A16, ldo=16, M=2, N=16, K=64, silu_in=0, silu_out=0)
SMALLM_SEG = dict(a=A16, lda=64, W=A16, bias=A16, out=A16, M=2, m0=0, Mtot=2, N=16, K=64, seg_start=SEG_PTR, nseg=2, silu_in=0, silu_out=0)
SMALLM_SEG_SPLIT = dict(a=A16, lda=64, W=A16, W_lo=A16, bias=A16, out=A16, M=2, m0=0, Mtot=2, N=16, K=64, seg_start=SEG_PTR, nseg=2, silu_in=0,
                        silu_out=0)
for entry, base in (("pnc_linear_smallm", SMALLM), ("pnc_linear_smallm_split", SMALLM_SPLIT), ("pnc_linear_smallm_segments", SMALLM_SEG),
                    ("pnc_linear_smallm_segments_split", SMALLM_SEG_SPLIT)):
    _each(entry, base, EINVAL, a=NULL, W=NULL, out=NULL, M=[0, 17], N=0, K=[0, 7, 68], lda=66)
    _each(entry, base, EALIGN, a=A8, W=A8)
    _row(entry, "order:K%8,a", _args(base, K=68, a=A8), EINVAL)
    if "W_lo" in base:
        _each(entry, base, EALIGN, W_lo=A8)
    if "nseg" in base:
        _each(entry, base, EINVAL, seg_start=NULL, m0=[-1, 1], Mtot=1, nseg=[0, 65])
        for tag, start, nseg in [("first!=0", (4, 8, 16), 2), ("last!=N", (0, 8, 12), 2), ("entry%4", (0, 6, 16), 2), ("not-ascending", (0, 8, 8, 16), 3),
                                 ("descending", (0, 12, 8, 16), 3)]:
            _row(entry, f"seg_start:{tag}", _args(base, seg_start=_segs(*start), nseg=nseg), EINVAL)
        _row(entry, "order:a,seg_start", _args(base, a=A8, seg_start=_segs(4, 8, 16)), EALIGN)      # the segment table is read last

# ---- embeddings, layout, elementwise, softmax ------------------------------------------------------------------------------------
T_EMB = dict(t=A16, F=2, dim=64, freqs=A16, out=A16)
TO_TOKENS = dict(a=A16, C1=4, a_scale=A16, a_frames=2, b=A16, C2=4, F=2, Npix=5, Cpad=8, out16=A16, out16_lo=A16)
TO_NCHW = dict(x=A16, ld=8, F=2, Npix=5, C=4, out=A16)
CONCAT_ADD = dict(a=A16, C1=8, s=A16, c=A16, C2=8, M=5, out32=A16, out16=A16, out16_lo=A16, lo_fmt=hip.LO_F16)
ADD = dict(x=A16, a=A16, n=64, y32=A16, y16=A16, y16_lo=A16, lo_fmt=hip.LO_F16)
CAST = dict(x=A16, n=64, y16=A16, y16_lo=A16, lo_fmt=hip.LO_F16)
SOFTMAX = dict(s=A16, lds=64, M=3, N=64, scale=0.125, causal=0, n_valid=0, p16=A16, ldp=64)
STATS = dict(hi=A16, lo=A16, lo_fmt=hip.LO_F16, rows=3, cols=64, ld=64, rec=A16)
for entry in ("pnc_timestep_embedding", "pnc_timestep_embedding_f32"):
    _each(entry, T_EMB, EINVAL, t=NULL, out=NULL, freqs=NULL, F=0, dim=1)
_each("pnc_nchw_to_tokens_f16", TO_TOKENS, EINVAL, a=NULL, out16=NULL, F=0, Npix=0, C1=0, C2=-1, b=NULL, a_frames=[0, 3], Cpad=[12, 0])
_each("pnc_nchw_to_tokens_f16", TO_TOKENS, EALIGN, out16=A8, out16_lo=A8)
_row("pnc_nchw_to_tokens_f16", "order:Cpad,out16", _args(TO_TOKENS, Cpad=12, out16=A8), EINVAL)
_each("pnc_tokens_to_nchw_f32", TO_NCHW, EINVAL, x=NULL, out=NULL, F=0, Npix=0, C=0, ld=3)
_each("pnc_concat_add", CONCAT_ADD, EINVAL, a=NULL, s=NULL, M=0, C1=[6, 0], C2=[6, 0], lo_fmt=2, out16=NULL)
_row("pnc_concat_add", "no-output", _args(CONCAT_ADD, out32=NULL, out16=NULL, out16_lo=NULL), EINVAL)
_each("pnc_add_f32", ADD, EINVAL, x=NULL, n=[0, 6], lo_fmt=2, y16=NULL)
_row("pnc_add_f32", "no-output", _args(ADD, y32=NULL, y16=NULL, y16_lo=NULL), EINVAL)
_each("pnc_cast_f16", CAST, EINVAL, x=NULL, n=[0, 6], lo_fmt=2, y16=NULL)
_row("pnc_cast_f16", "no-output", _args(CAST, y16=NULL, y16_lo=NULL), EINVAL)
_each("pnc_softmax_rows_f16", SOFTMAX, EINVAL, s=NULL, p16=NULL, M=0, N=[0, 66, 16388], n_valid=65, lds=[66, 32], ldp=[66, 32])
_each("pnc_softmax_rows_f16", SOFTMAX, EALIGN, s=A8, p16=A2)
_row("pnc_softmax_rows_f16", "order:lds,s", _args(SOFTMAX, lds=66, s=A8), EINVAL)
_row("pnc_softmax_rows_f16", "order:n_valid,p16", _args(SOFTMAX, n_valid=65, p16=A2), EINVAL)

# ---- pnc_operand_stats_f16 (stats.hip), the range monitor, the options -------------------------------------------------------------
_each("pnc_operand_stats_f16", STATS, EINVAL, hi=NULL, rec=NULL, rows=0, cols=0, ld=56, lo_fmt=2)
_row("pnc_operand_stats_f16", "rows*ld>=2^59", _args(STATS, rows=1 << 54), EINVAL)                 # byte offsets leave int64
_row("pnc_operand_stats_f16", "chunks>2^40", _args(STATS, rows=1 << 38), EINVAL)                   # a wave's 32-bit counters
_each("pnc_operand_stats_f16", STATS, EALIGN, cols=60, ld=68, hi=A8, rec=A2, lo=A8)
_row("pnc_operand_stats_f16", "e4m3-lo&7", _args(STATS, lo_fmt=hip.LO_E4M3, lo=A2), EALIGN)
_row("pnc_operand_stats_f16", "order:lo_fmt,cols", _args(STATS, lo_fmt=2, cols=60), EINVAL)            # arguments before alignment
_row("pnc_operand_stats_f16", "order:rows,ld%8", _args(STATS, rows=1 << 54, ld=68), EINVAL)
_row("pnc_operand_stats_f16", "order:rows-chunks,hi", _args(STATS, rows=1 << 38, hi=A8), EINVAL)
_row("pnc_range_monitor_collect", "out=NULL", (None, None), EINVAL)
for option in (-1, 12):                                            # PNC_OPT_COUNT = 12; an accepted call returns the previous value
    _row("pnc_set_option", f"option={option}", (option, 0), EINVAL)


@pytest.mark.parametrize("entry,args,want", ROWS)
def test_rejected_before_any_launch(entry, args, want):
    assert want < 0                       # only rejecting rows reach a launching entry point
    args = tuple(C.byref(a) if isinstance(a, C.Structure) else a for a in args)
    assert getattr(hip.load(), entry)(*args) == want


def test_the_base_arguments_are_the_entry_points_own():
    """the ordered base dicts above have one value per parameter of their entry point (the stream is added by _args)"""
    for entry, base in (("pnc_attn_temporal_f16", TEMPORAL), ("pnc_attn_temporal_split_f16", TEMPORAL_SPLIT), ("pnc_groupnorm_stats", GN_STATS),
                        ("pnc_concat_add_stats", CONCAT), ("pnc_groupnorm_apply", GN_APPLY), ("pnc_groupnorm_combine", GN_COMBINE),
                        ("pnc_groupnorm_temporal_silu", GN_T_SILU), ("pnc_groupnorm_temporal_part", GN_T_PART), ("pnc_layernorm", LAYERNORM),
                        ("pnc_cfg_euler_step", EULER), ("pnc_cfg_euler_step_skip", EULER_SKIP), ("pnc_linear_smallm", SMALLM),
                        ("pnc_linear_smallm_split", SMALLM_SPLIT), ("pnc_linear_smallm_segments", SMALLM_SEG),
                        ("pnc_linear_smallm_segments_split", SMALLM_SEG_SPLIT), ("pnc_timestep_embedding", T_EMB),
                        ("pnc_timestep_embedding_f32", T_EMB), ("pnc_nchw_to_tokens_f16", TO_TOKENS), ("pnc_tokens_to_nchw_f32", TO_NCHW),
                        ("pnc_concat_add", CONCAT_ADD), ("pnc_add_f32", ADD), ("pnc_cast_f16", CAST), ("pnc_softmax_rows_f16", SOFTMAX),
                        ("pnc_operand_stats_f16", STATS)):
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
