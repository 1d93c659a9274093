"""Cases of the helper and row-softmax tests (tests/test_misc_edges_gpu.py on the MI355X, tests/test_misc_ref64.py on the CPU): sections 4
and 5 of include/panacea_hip.h at the shapes where their loops and guards change behaviour.

A case is one launch (the two-part segment cases: the two launches that fill one output) in one of its data sets.  Every operand is a
16-byte-aligned VIEW inside a larger allocation whose every other element is poison — NaN for fp16 / fp32, 0xFF for e4m3 bytes, 2^62
for int64 timesteps: MARGIN elements in front and behind, every leading-dimension gap (lda > K, ldo > N, lds > N, ldp > N, ld > C), and
the padding columns N .. lds - 1 of a score matrix.  Every output holds poison before the launch.  A launch that reads an element its
contract does not name drags a NaN into a value; one that writes such an element changes the poison's bits.  Nothing outside an
allocation is addressed by a correct or a slightly wrong kernel: the shapes are ordinary and no case is shaped to provoke a fault.

Shapes (why these):
  linears     K in {8, 72, 512, 520, 1288}: one lane / nine lanes / exactly one K round of the 64 x 8 lane stride / one round + one lane /
              two rounds + a ragged third; N in {1, 5, 320}: less than a workgroup's four waves, a ragged second workgroup, many; M in
              {1, 7, 16}; lda = K + 4, ldo = N + 3.  Segments: widths [4, 8, 64] and [320, 4] (a one-wave site first and last), Mtot = 21
              written as rows 0..15 then 16..20.
  embeddings  dim in {2, 7, 320} (one frequency; odd: the zero column; the product's), F in {1, 5}.
  layout      Npix in {1, 77, 257}: one lane, a partly filled workgroup, one workgroup + one lane.
  softmax     SOFTMAX_SHAPES: rows beyond N under a causal mask, ldp != lds, one visible key, 1028 = 257 float4 (a
              second register round of ONE lane), the 16384-column limit on 3 rows, 64 rows of a causal + n_valid launch.
"""
import math
import zlib

import torch

import misc_ref64 as ref64

NAN = float("nan")
MARGIN = 256
T_POISON = 2 ** 62
SPECIALS = [700.24, 0.0, 2.0 ** -14, 1e-6, 700.0, -1200.0, 60000.0, -1200.4, 60007.3]     # |v| >= 512 off the fp16 grid: the e4m3 lo plane clamps


def _poison(dtype):
    return 0xFF if dtype == torch.uint8 else T_POISON if dtype == torch.int64 else NAN


class Plane:
    """a 1-D body inside [MARGIN poison | body | MARGIN poison]"""

    def __init__(self, body):
        body = body.reshape(-1)
        self.n = body.numel()
        self.alloc = torch.full((self.n + 2 * MARGIN,), _poison(body.dtype), dtype=body.dtype)
        self.alloc[MARGIN:MARGIN + self.n] = body

    def view(self, alloc):
        return alloc[MARGIN:MARGIN + self.n]


def strided(mat, ld):
    """[R, C] -> flat (R - 1) * ld + C elements, row r at r * ld, the gaps poisoned"""
    R, C = mat.shape
    flat = torch.full(((R - 1) * ld + C,), _poison(mat.dtype), dtype=mat.dtype)
    torch.as_strided(flat, (R, C), (ld, 1)).copy_(mat)
    return flat


def blank(n, dtype=torch.float32):
    return torch.full((n,), _poison(dtype), dtype=dtype)


LO_DTYPE = {"f16": torch.float16, "e4m3": torch.uint8}


class Case:
    def __init__(self, name, family, fn, data, **spec):
        self.name, self.family, self.fn, self.data, self.spec = name, family, fn, data, spec
        self._built, self._ref = {}, {}

    def __repr__(self):
        return self.name

    def build(self, data):
        """-> (ins {name: Plane}, outs {name: Plane as it starts}, alias {operand name: output name it IS})"""
        if data not in self._built:
            # (the data sets of a softmax case share their draws: "masked-nonfinite" is "randn30" with other masked columns)
            g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()) % (2 ** 31) + (0 if self.fn == "softmax" else self.data.index(data)))
            self._built[data] = _BUILD[self.fn](self.spec, data, g)
        return self._built[data]

    def launch(self, data, device=None, zero_poison=False):
        """-> ({name: fresh view} of every operand and output, {output name: its whole allocation}).  zero_poison: the operands' poison
        replaced by zeros (the reference must not notice)"""
        ins, outs, alias = self.build(data)
        t, allocs = {}, {}
        for n, pl in outs.items():
            allocs[n] = pl.alloc.clone() if device is None else pl.alloc.to(device)
            t[n] = pl.view(allocs[n])
        for n, pl in ins.items():
            a = pl.alloc.clone()
            if zero_poison:
                body = pl.view(a)
                body[(body == _poison(a.dtype)) if a.dtype in (torch.uint8, torch.int64) else torch.isnan(body)] = 0
                a[:MARGIN], a[MARGIN + pl.n:] = 0, 0
            t[n] = pl.view(a if device is None else a.to(device))
        for n, o in alias.items():
            t[n] = t[o]
        return t, allocs

    def call(self, mod, t, **over):
        """the launch on `mod` (panacea_amd.hip or tests/emu.py) with the tensors of launch(); `over` replaces spec entries"""
        _CALL[self.fn](mod, dict(self.spec, **over), t)

    def reference(self, data):
        """-> ({output name: misc_ref64.Expect}, clamped e4m3 quads), computed once from the CPU operands and left unchanged"""
        if data not in self._ref:
            self._ref[data] = _REF[self.fn](self.spec, self.launch(data)[0])
        return self._ref[data]


def _rand(g, data, *shape, scale=1.0, offset=0.5):
    x = torch.randn(*shape, generator=g)
    return (x.abs() + offset if data == "positive" else x) * scale


# ------------------------------------------------------------------------------------------------------------------------- linears
def _build_linear(s, data, g):
    K, N, Mtot = s["K"], s["N"], s["Mtot"]
    lda = K + 4
    a = _rand(g, data, Mtot, K, scale=8.0 if s.get("big") else 1.0)
    if s.get("big"):                                     # activations reaching +-30 under silu_in
        a[0, 0], a[0, 1], a[-1, -1] = 30.0, -30.0, -30.0 if data == "signed" else 30.0
        a.clamp_(-30.0, 30.0)
    ins = dict(a32=Plane(strided(a, lda)), w16=Plane(_rand(g, data, N, K, scale=K ** -0.5, offset=0.0).half()))
    if s.get("w_lo"):
        lo = (torch.rand(N, K, generator=g) * 2.0 - 1.0) * 1024.0
        lo[0, 0] = 1024.0
        ins["w_lo"] = Plane((lo.abs() if data == "positive" else lo).half())
    if s["bias"]:
        ins["bias"] = Plane(_rand(g, data, N))
    n_out = N * Mtot if s.get("segs") else (Mtot - 1) * (N + 3) + N
    return ins, dict(out32=Plane(blank(n_out))), {}


def _linear_parts(s):
    return s.get("parts") or [(0, s["Mtot"])]


def _call_linear(mod, s, t):
    K, N, lda = s["K"], s["N"], s["K"] + 4
    kw = dict(silu_in=s.get("silu_in", False), silu_out=s.get("silu_out", False), w_lo=t.get("w_lo"))
    for m0, M in _linear_parts(s):
        a = t["a32"][m0 * lda:]
        if s.get("segs"):
            mod.linear_smallm_segments(a, lda, t["w16"], t.get("bias"), t["out32"], M, m0, s["Mtot"], N, K, _starts(s["segs"]), **kw)
        else:
            mod.linear_smallm(a, lda, t["w16"], t.get("bias"), t["out32"], N + 3, M, N, K, **kw)


def _starts(widths):
    out = [0]
    for w in widths:
        out.append(out[-1] + w)
    return out


def _ref_linear(s, t):
    K, N, lda = s["K"], s["N"], s["K"] + 4
    kw = dict(silu_in=s.get("silu_in", False), silu_out=s.get("silu_out", False), w_lo=t.get("w_lo"))
    parts = []
    for m0, M in _linear_parts(s):
        a = t["a32"][m0 * lda:]
        if s.get("segs"):
            parts.append(ref64.linear_smallm_segments(a, lda, t["w16"], t.get("bias"), M, m0, s["Mtot"], N, K, _starts(s["segs"]), **kw)["out32"])
        else:
            parts.append(ref64.linear_smallm(a, lda, t["w16"], t.get("bias"), N + 3, M, N, K, **kw)["out32"])
    cat = [torch.cat([getattr(p, f) for p in parts]) for f in ("idx", "v", "floor", "allow")]
    return {"out32": ref64.Expect(cat[0], cat[1], floor=cat[2], allow=cat[3])}, 0


def _linear_cases():
    out, i = [], 0
    d = ("signed", "positive")
    for K in (8, 72, 512, 520, 1288):
        for N in (1, 5, 320):
            for M in (1, 7, 16):
                out.append(Case(f"linear-K{K}-N{N}-M{M}-{'bias' if i % 2 == 0 else 'nobias'}", "linear", "linear", d, K=K, N=N, Mtot=M, bias=i % 2 == 0))
                i += 1
    for si in (0, 1):
        for so in (0, 1):
            out.append(Case(f"linear-K520-N5-M7-silu{si}{so}-pm30", "linear silu", "linear", d, K=520, N=5, Mtot=7, bias=True, silu_in=si,
                            silu_out=so, big=True))
    out.append(Case("linear-K1288-N320-M16-silu10-pm30", "linear silu", "linear", d, K=1288, N=320, Mtot=16, bias=True, silu_in=1, silu_out=0, big=True))
    for K, N, M, bias in ((8, 1, 1, False), (520, 5, 7, True), (1288, 320, 16, True)):
        out.append(Case(f"linear-K{K}-N{N}-M{M}-wlo", "linear split", "linear", d, K=K, N=N, Mtot=M, bias=bias, w_lo=True))
    for widths in ([4, 8, 64], [320, 4]):
        tag = "+".join(map(str, widths))
        for K in (72, 520):
            for w_lo in (False, True):
                out.append(Case(f"segments-{tag}-K{K}-Mtot21{'-wlo' if w_lo else ''}", "linear segments", "linear", d, K=K, N=sum(widths), Mtot=21,
                                bias=True, segs=widths, parts=[(0, 16), (16, 5)], w_lo=w_lo, silu_in=1))
        out.append(Case(f"segments-{tag}-K8-M1-nobias", "linear segments", "linear", d, K=8, N=sum(widths), Mtot=1, bias=False, segs=widths))
    return out


# ---------------------------------------------------------------------------------------------------------------------- embeddings
T_INT = [0, 1, 999, 2 ** 24 + 1]
T_FLOAT = [-1.7, 0.25 * math.log(0.002), 999.0, 0.5]


def freqs_table(dim, max_period=10000.0):
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half)


def _build_embed(s, data, g):
    t = torch.tensor(s["t"], dtype=torch.int64 if s["kind"] == "i64" else torch.float32)
    return dict(t=Plane(t), freqs=Plane(freqs_table(s["dim"]))), dict(out32=Plane(blank(s["F"] * s["dim"]))), {}


def _call_embed(mod, s, t):
    fn = mod.timestep_embedding if t["t"].dtype == torch.int64 else mod.timestep_embedding_f32
    fn(t["t"], s["F"], s["dim"], t["freqs"], t["out32"])


def _ref_embed(s, t):
    return ref64.timestep_embedding(t["t"], s["F"], s["dim"], t["freqs"]), 0


def _embed_cases():
    out = []
    for kind, ts in (("i64", T_INT), ("f32", T_FLOAT)):
        for dim in (2, 7, 320):
            for k, tv in enumerate(ts):
                out.append(Case(f"embed-{kind}-dim{dim}-F1-t{k}", "embedding", "embed", ("t",), kind=kind, dim=dim, F=1, t=[tv]))
            out.append(Case(f"embed-{kind}-dim{dim}-F5", "embedding", "embed", ("t",), kind=kind, dim=dim, F=5, t=ts + ts[2:3]))
    return out


# -------------------------------------------------------------------------------------------------------------------------- layout
def _with_specials(x, values=SPECIALS):
    flat = x.reshape(-1)
    n = min(flat.numel(), len(values))
    flat[:n] = torch.tensor(values[:n])
    return x


def _build_nchw(s, data, g):
    F, af, C1, C2, Npix, Cpad = s["F"], s["af"], s["C1"], s["C2"], s["Npix"], s["Cpad"]
    ins = dict(a32=Plane(_with_specials(torch.randn(af * C1 * Npix, generator=g) * 3.0, SPECIALS[:6])))      # (times a_scale: inside fp16)
    if s["scale"]:
        ins["a_scale"] = Plane(0.5 + torch.rand(F, generator=g) + torch.arange(F) * 0.25)
    if C2:
        ins["b32"] = Plane(_with_specials(torch.randn(F * C2 * Npix, generator=g) * 3.0))
    outs = dict(out16=Plane(blank(F * Npix * Cpad, torch.float16)))
    if s["lo"]:
        outs["out16_lo"] = Plane(blank(F * Npix * Cpad, torch.float16))
    return ins, outs, {}


def _call_nchw(mod, s, t):
    mod.nchw_to_tokens_f16(t["a32"], s["C1"], t.get("b32"), s["C2"], s["F"], s["Npix"], s["Cpad"], t["out16"], t.get("out16_lo"),
                           a_scale=t.get("a_scale"), a_frames=s["af"])


def _ref_nchw(s, t):
    return ref64.nchw_to_tokens_f16(t["a32"], s["C1"], t.get("a_scale"), s["af"], t.get("b32"), s["C2"], s["F"], s["Npix"], s["Cpad"], s["lo"]), 0


def _nchw_cases():
    out, i = [], 0
    chans = [(4, 0, 8), (4, 4, 8), (4, 4, 24), (19, 0, 24), (19, 4, 24), (4, 0, 24)]          # C1, C2, Cpad
    for F, af in ((4, 2), (3, 3), (2, 1)):
        for scale in (True, False):
            for Npix in (1, 77, 257):
                for k in (0, 3):
                    C1, C2, Cpad = chans[(i + k) % 6]
                    lo = (i // 2 + k) % 2 == 0
                    out.append(Case(f"nchw-F{F}-af{af}-{'scale' if scale else 'noscale'}-C{C1}+{C2}-pad{Cpad}-Npix{Npix}{'-lo' if lo else ''}",
                                    "nchw_to_tokens", "nchw", ("v",), F=F, af=af, scale=scale, C1=C1, C2=C2, Cpad=Cpad, Npix=Npix, lo=lo))
                i += 1
    return out


def _build_tok(s, data, g):
    F, C, ld, Npix = 2, s["C"], s["ld"], s["Npix"]
    x = _with_specials(torch.randn(F * Npix, C, generator=g))
    return dict(x32=Plane(strided(x, ld))), dict(out32=Plane(blank(F * C * Npix))), {}


def _call_tok(mod, s, t):
    mod.tokens_to_nchw_f32(t["x32"], s["ld"], 2, s["Npix"], s["C"], t["out32"])


def _ref_tok(s, t):
    return ref64.tokens_to_nchw_f32(t["x32"], s["ld"], 2, s["Npix"], s["C"]), 0


def _tok_cases():
    return [Case(f"tokens_to_nchw-C{C}-ld{C + pad}-Npix{Npix}", "tokens_to_nchw", "tok", ("v",), C=C, ld=C + pad, Npix=Npix)
            for C in (1, 4) for pad in (0, 5) for Npix in (1, 257)]


# --------------------------------------------------------------------------------------------------------------------- elementwise
def _cast_outs(n, s, first=None):
    outs = {}
    if s["o32"]:
        outs["out32"] = Plane(blank(n) if first is None else first)
    outs["out16"] = Plane(blank(n, torch.float16))
    if s["lo"]:
        outs["out16_lo"] = Plane(blank(n, LO_DTYPE[s["lo"]]))
    return outs


def _build_concat(s, data, g):
    C1, C2, M = s["C1"], s["C2"], s["M"]
    ins = dict(a32=Plane(_with_specials(torch.randn(M * C1, generator=g) * 5.0)), s32=Plane(_with_specials(torch.randn(M * C2, generator=g))))
    if s["c"]:
        ins["c32"] = Plane(torch.randn(M * C2, generator=g))
    return ins, _cast_outs(M * (C1 + C2), s), {}


def _call_concat(mod, s, t):
    mod.concat_add(t["a32"], s["C1"], t["s32"], t.get("c32"), s["C2"], s["M"], t.get("out32"), t["out16"], t.get("out16_lo"))


def _ref_concat(s, t):
    return ref64.concat_add(t["a32"], s["C1"], t["s32"], t.get("c32"), s["C2"], s["M"], s["o32"], True, s["lo"])


def _concat_cases():
    out = []
    variants = [(1, 1, "f16"), (0, 1, "e4m3"), (1, 0, "e4m3"), (0, 0, "f16"), (1, 1, None), (1, 1, "e4m3")]        # c, out32, lo
    for C1 in (4, 68):
        for C2 in (4, 68):
            for M in (1, 300):
                for c, o32, lo in variants:
                    out.append(Case(f"concat-C{C1}+{C2}-M{M}-{'c' if c else 'noc'}-{'o32' if o32 else 'no32'}-lo{lo}", "concat_add", "concat", ("v",),
                                    C1=C1, C2=C2, M=M, c=c, o32=o32, lo=lo))
    return out


def _build_add(s, data, g):
    n = s["n"]
    x = _with_specials(torch.randn(n, generator=g) * 5.0)
    ins, alias = {}, {}
    if s["add"]:
        a = torch.randn(n, generator=g)
        a[: min(n, len(SPECIALS))] = 0.0              # the special values reach the casts as they are
        ins["a32"] = Plane(a)
    if s["inplace"]:
        alias["x32"] = "out32"                          # y32 == x: the output starts as x
    else:
        ins["x32"] = Plane(x)
    return ins, _cast_outs(n, s, first=x if s["inplace"] else None), alias


def _call_add(mod, s, t):
    if s["add"]:
        mod.add_f32(t["x32"], t["a32"], s["n"], t.get("out32"), t["out16"], t.get("out16_lo"))
    else:
        mod.cast_f16(t["x32"], s["n"], t["out16"], t.get("out16_lo"))


def _ref_add(s, t):
    return ref64.add_f32(t["x32"], t.get("a32"), s["n"], s["o32"], True, s["lo"])


def _add_cases():
    out = []
    for n in (4, 1028):
        for lo in (None, "f16", "e4m3"):
            for inplace in (True, False):
                out.append(Case(f"add-n{n}-lo{lo}{'-inplace' if inplace else ''}", "add_f32", "add", ("v",), n=n, lo=lo, add=True, inplace=inplace, o32=True))
            out.append(Case(f"cast-n{n}-lo{lo}", "cast_f16", "add", ("v",), n=n, lo=lo, add=False, inplace=False, o32=False))
    return out


# ------------------------------------------------------------------------------------------------------------------------- softmax
SOFTMAX_SHAPES = [(9, 4, 8, 12, 0, 1), (5, 80, 80, 88, 77, 0), (7, 1000, 1024, 1000, 1, 0), (6, 1028, 1028, 1032, 1000, 1),
                  (3, 16384, 16384, 16384, 0, 0), (64, 256, 256, 256, 200, 1)]                 # M, N, lds, ldp, n_valid, causal
SOFTMAX_SCALES = [0.125, 1.0, 512 ** -0.5, 0.0, 1e-38]
SOFTMAX_DATA = ("randn30", "spike", "equal", "offset", "masked-nonfinite")


def visible(M, N, n_valid, causal):
    m, j = torch.arange(M).view(M, 1), torch.arange(N).view(1, N)
    return (j < (n_valid if n_valid > 0 else N)) & ((j <= m) if causal else torch.ones(M, N, dtype=torch.bool))


def _build_softmax(s, data, g):
    M, N, lds, ldp = s["M"], s["N"], s["lds"], s["ldp"]
    x = torch.randn(M, N, generator=g) * 30.0             # (the same draws for every data set of a case: the generator starts here)
    if data == "spike":                                    # + 400 in one VISIBLE column per row (column 0 is visible in every row)
        vis = visible(M, N, s["n_valid"], s["causal"])
        col = (torch.arange(M) * 7919) % N
        col = torch.where(vis[torch.arange(M), col], col, torch.zeros_like(col))
        x[torch.arange(M), col] += 400.0
    elif data == "equal":
        x = x[:, :1].expand(M, N).clone()
    elif data == "offset":
        x = x + 1.0e4
    elif data == "masked-nonfinite":                       # "randn30" with NaN / +Inf / -Inf in every masked column
        vis = visible(M, N, s["n_valid"], s["causal"])
        junk = torch.tensor([NAN, math.inf, -math.inf])[(torch.arange(M).view(M, 1) + torch.arange(N).view(1, N)) % 3]
        x = torch.where(vis, x, junk)
    return dict(s32=Plane(strided(x, lds))), dict(p16=Plane(blank((M - 1) * ldp + N, torch.float16))), {}


def _call_softmax(mod, s, t):
    mod.softmax_rows(t["s32"], s["lds"], s["M"], s["N"], s["scale"], t["p16"], s["ldp"], causal=bool(s["causal"]), n_valid=s["n_valid"])


def _ref_softmax(s, t):
    return ref64.softmax_rows(t["s32"], s["lds"], s["M"], s["N"], s["scale"], s["causal"], s["n_valid"], s["ldp"]), 0


def _softmax_cases():
    out = []
    for M, N, lds, ldp, nv, causal in SOFTMAX_SHAPES:
        masked = nv > 0 or causal
        data = tuple(d for d in SOFTMAX_DATA if masked or d != "masked-nonfinite")
        pad = f"-lds{lds}-pad_never_read" if lds > N else ""
        for scale in SOFTMAX_SCALES:
            name = f"softmax-M{M}-N{N}{pad}-ldp{ldp}-nv{nv}-{'causal' if causal else 'full'}-scale{scale:.3g}" + ("-masked_cols_arbitrary" if masked else "")
            out.append(Case(name, "softmax", "softmax", data, M=M, N=N, lds=lds, ldp=ldp, n_valid=nv, causal=causal, scale=scale))
    return out


_BUILD = dict(linear=_build_linear, embed=_build_embed, nchw=_build_nchw, tok=_build_tok, concat=_build_concat, add=_build_add, softmax=_build_softmax)
_CALL = dict(linear=_call_linear, embed=_call_embed, nchw=_call_nchw, tok=_call_tok, concat=_call_concat, add=_call_add, softmax=_call_softmax)
_REF = dict(linear=_ref_linear, embed=_ref_embed, nchw=_ref_nchw, tok=_ref_tok, concat=_ref_concat, add=_ref_add, softmax=_ref_softmax)

CASES = _linear_cases() + _embed_cases() + _nchw_cases() + _tok_cases() + _concat_cases() + _add_cases() + _softmax_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c, d) for c in CASES for d in c.data]
RUN_IDS = [f"{c.name}[{d}]" for c, d in RUNS]


# ------------------------------------------------------------------------------------------------------------------- the checks
def bits(t):
    return t.view({torch.float32: torch.int32, torch.float16: torch.int16, torch.uint8: torch.uint8, torch.int64: torch.int64}[t.dtype])


def check_outputs(case, data, expects, t, allocs, share=1.0):
    """What every launch of a case has to satisfy, for the tensors `t` / `allocs` of Case.launch after the launch (any device): every
    element the reference marks as written equals the expectation bit for bit (exact outputs) or is finite and within floor + share *
    allow of the float64 value — no element is skipped; where that bound is 0 the output is +0 — and every other element of every
    output allocation (margins, leading-dimension gaps) holds the bits it started with.  -> {output: worst err / bound};
    raises AssertionError naming the case, the first bad index and err / bound."""
    tag = f"{case.name} [{data}]"
    worst = {}
    start = case.build(data)[1]
    for name, ex in expects.items():
        flat = t[name].reshape(-1).cpu()
        if ex.exact is not None:
            got = flat[ex.idx]
            bad = bits(got) != bits(ex.exact)
            assert not bad.any(), f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at " \
                                  f"{torch.nonzero(bad)[0].tolist()}: got {got[bad][0].item()!r}, want {ex.exact[bad][0].item()!r}"
            worst[name] = 0.0
            continue
        got = flat.double()[ex.idx]
        bad = ~torch.isfinite(got)
        assert not bad.any(), f"{tag} {name}: {int(bad.sum())} of {got.numel()} written elements are not finite, first at {torch.nonzero(bad)[0].tolist()}"
        b, err = ex.bound(share), (got - ex.v).abs()
        zero = b == 0
        notzero = zero & (bits(flat)[ex.idx] != 0)
        assert not notzero.any(), f"{tag} {name}: {int(notzero.sum())} elements that must be +0 are not, first at {torch.nonzero(notzero)[0].tolist()}: " \
                                  f"got {got[notzero][0].item()!r}"
        ratio = torch.where(zero, torch.zeros_like(err), err / b.clamp_min(1e-300))
        worst[name] = ratio.max().item()
        if worst[name] > 1.0:
            at = tuple(torch.nonzero(ratio > 1.0)[0].tolist())
            raise AssertionError(f"{tag} {name}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements outside the bound, worst err / bound "
                                 f"{worst[name]:.3g}; first bad {at}: got {got[at].item():.9g}, float64 {ex.v[at].item():.9g}, bound {b[at].item():.3g}")
    for name, alloc in allocs.items():
        written = torch.zeros(alloc.numel(), dtype=torch.bool)
        written[MARGIN + expects[name].idx.reshape(-1)] = True
        touched = (bits(alloc.cpu()) != bits(start[name].alloc)) & ~written
        assert not touched.any(), f"{tag} {name}: {int(touched.sum())} elements outside the written set changed, first at element " \
                                  f"{int(torch.nonzero(touched)[0]) - MARGIN} of the view"
    return worst
