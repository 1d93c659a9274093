"""Operand builders of the GEMM edge cases (tests/test_gemm_edges_gpu.py on the MI355X, tests/test_gemm_ref64.py on the CPU).

A case is one launch: the keywords shared by hip.gemm, emu.gemm and
gemm_ref64.gemm.  Every plane — A, A_lo, W, W_lo, bias, rowbias, res1, res2 and every output — is a 16-byte-aligned VIEW inside a
larger allocation whose every other element is poison: NaN for fp16 / fp32, 0xFF (the e4m3 NaN code) for e4m3 bytes.  MARGIN = 256
poisoned elements sit in front of the view and behind it, every leading-dimension gap (lda > K, w_ld > K, ldr > N, ldc > N, ldt >
t_rows) is poisoned, and so is everything between a band and its x_halo_off column block.  A launch that reads an element its
contract does not name multiplies it into an accumulator (0 x NaN = NaN) and is seen; a launch that writes one changes the poison's
bits and is seen.  Nothing outside an allocation is ever addressed by a correct or by a slightly wrong kernel: the shapes are
ordinary, the margins are wider than any tile's over-read of a row, and no case is shaped to provoke a fault.

Data sets: `signed` — randn activations, randn * K^-0.5 weights; `positive` — |randn| + 0.5 activations and |randn| * K^-0.5 weights,
for which gemm_ref64's `mag` ~ |ref| and its bound is a relative one.  fp32 streams follow the sign convention of the set.
Both are unit scale; RANGE_CASES on RANGE_DATA (`wide-rows`, `graded-cols`, each with a positive variant; "over the range" below;
tests/test_gemm_range_gpu.py, tests/test_gemm_range_ref64.py) walk the number range on the same machinery.

Not here: the persistent kernels (PNC_OPT_GEMM_PERSIST bits 0 and 1).  They need at least 512 whole tiles — far beyond a quick test —
and tests/test_kernels_gpu.py already pins them bit for bit to the one-tile-per-workgroup kernels these cases run."""
import zlib

import torch

import gemm_ref64
import misc_ref64
from panacea_amd import engine

A_PLAIN, A_CONV3X3, A_CONV1D_T = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
NAN = float("nan")
MARGIN = 256
DATA = ("signed", "positive")
# the operand RANGE (see "over the range" below); a trailing + = the positive variant.  A case of RANGE_CASES belongs to one family
RANGE_DATA = ("wide-rows", "wide-rows+", "graded-cols", "graded-cols+")
_ALL_DATA = DATA + RANGE_DATA
_POSITIVE = ("positive", "wide-rows+", "graded-cols+")
E_LO, E_HI = -24, 13         # wide-rows: the binades storage row i of A walks, E_LO + i % (E_HI - E_LO + 1)
G_WALK = (-20, -8, 0, 5, 12)  # wide-rows: the weights' 2^g over the case list


class Plane:
    """a 1-D body inside [MARGIN poison | body | MARGIN poison]; `shape`: the view handed to the launch (default flat)"""

    def __init__(self, body, shape=None):
        body = body.reshape(-1)
        self.n, self.shape = body.numel(), shape
        self.alloc = torch.full((self.n + 2 * MARGIN,), 0xFF if body.dtype == torch.uint8 else NAN, dtype=body.dtype)
        self.alloc[MARGIN:MARGIN + self.n] = body

    def view(self, alloc):
        v = alloc[MARGIN:MARGIN + self.n]
        return v if self.shape is None else v.view(self.shape)


def strided(mat, ld):
    """[R, C] -> flat (R - 1) * ld + C elements, row r at r * ld, the gaps poisoned"""
    R, C = mat.shape
    flat = torch.full(((R - 1) * ld + C,), NAN, dtype=mat.dtype)
    torch.as_strided(flat, (R, C), (ld, 1)).copy_(mat)
    return flat


def split_planes(v32, fmt):
    """fp32 (NaN = poison) -> (hi fp16, lo plane in `fmt` or None) with the poison kept in both"""
    hi = v32.half()
    if fmt is None:
        return hi, None
    r = (v32 - hi.float()) * 2048.0
    if fmt == "f16":
        return hi, r.half()
    q = r.nan_to_num(0.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).clone()
    q[torch.isnan(v32)] = 0xFF
    return hi, q


class Case:
    def __init__(self, name, family, spec):
        self.name, self.family, self.spec = name, family, spec
        self.K = spec["K"]
        self.opts = spec.get("opts", {})
        self._built = {}
        self.top = {}              # graded-cols: the top grade per data set, found from the reference (build)

    def __repr__(self):
        return self.name

    def build(self, data):
        """-> (kw: non-tensor keywords, planes: {keyword: Plane} operands, outs: {keyword: Plane} outputs as they start, alias: {operand
        keyword: output keyword it aliases}, w_lo_exp or None)"""
        if data not in self._built:
            if data.startswith("graded-cols"):
                # the largest integer top grade for which the REFERENCE's max |v| stays below 32768 (fp16 lo planes stay finite)
                for top in range(15, E_LO, -1):
                    built = _build(self.name, self.spec, data, top)
                    if gemm_ref64.gemm(**_tensors(built)[0])["v"].abs().max() < 32768.0:
                        break
                else:
                    raise AssertionError(f"{self.name}: no top grade keeps the reference below 32768")
                self.top[data] = top
                self._built[data] = built
            else:
                self._built[data] = _build(self.name, self.spec, data)
        return self._built[data]

    def launch(self, data, device=None, zero_poison=False):
        """-> (keywords for hip.gemm / emu / gemm_ref64 with fresh tensors, {output keyword: whole allocation}).  zero_poison: the
        operands' poison replaced by zeros (the reference must not notice)"""
        return _tensors(self.build(data), device, zero_poison)


def _tensors(built, device=None, zero_poison=False):
    """Case.launch for the tuple `_build` returns"""
    kw, planes, outs, alias, w_exp = built
    kw = dict(kw)
    allocs = {}
    for n, pl in outs.items():
        allocs[n] = pl.alloc.clone() if device is None else pl.alloc.to(device)
        kw[n] = pl.view(allocs[n])
    for n, pl in planes.items():
        a = pl.alloc
        if zero_poison:
            a = a.clone()
            a[(a == 0xFF) if a.dtype == torch.uint8 else torch.isnan(a)] = 0          # (no datum is the e4m3 NaN code)
        t = pl.view(a if device is None else a.to(device))
        kw[n] = (t, w_exp) if n == "w_lo" and w_exp is not None else t
    for n, o in alias.items():
        kw[n] = kw[o]
    return kw, allocs


def _rand(g, data, *shape, scale=1.0, offset=0.5):
    x = torch.randn(*shape, generator=g)
    return (x.abs() + offset if data in _POSITIVE else x) * scale


def _wide(g, data, rows, cols):
    """wide-rows: storage row i (a row of a plain A, a pixel of a conv gather) in binade E_LO + i % 38, sign (1 + rand) 2^e"""
    e = E_LO + torch.arange(rows) % (E_HI - E_LO + 1)
    x = (1.0 + torch.rand(rows, cols, generator=g)) * torch.exp2(e.float()).view(rows, 1)
    return x if data in _POSITIVE else x * (torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1).float()


def _grades(s, top):
    """graded-cols: (2^grade per column of `pre` [N], 2^grade per column of the OUTPUT [No]).  The output grade walks linearly from
    E_LO to `top`; under GEGLU the `value` blocks carry it and the `gate` blocks walk [-3, 5] (gates beyond the table's [-8, 8))"""
    N = s["N"]
    if "geglu" not in s["epi"].split("+"):
        sc = torch.exp2(E_LO + (top - E_LO) * torch.arange(N, dtype=torch.float64) / (N - 1)).float()
        return sc, sc
    No = N // 2
    j = torch.arange(No, dtype=torch.float64) / (No - 1)
    val, gate = torch.exp2(E_LO + (top - E_LO) * j).float(), torch.exp2(-3.0 + 8.0 * j).float()
    return torch.stack([val.view(No // 32, 32), gate.view(No // 32, 32)], dim=1).reshape(N), val


def _build(name, s, data, top=None):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2 ** 31) + _ALL_DATA.index(data))
    M, N, K = s["M"], s["N"], s["K"]
    epi = set(s["epi"].split("+"))
    mode = s["mode"]
    kw = dict(M=M, N=N, K=K, a_mode=mode)
    wide = data.startswith("wide-rows")
    pre_sc, out_sc = _grades(s, top) if data.startswith("graded-cols") else (1.0, 1.0)
    # ---- A
    if mode == A_PLAIN:
        lda = s.get("lda", K + 8)
        a32 = strided(_wide(g, data, M, K) if wide else _rand(g, data, M, K), lda)
        kw["lda"] = lda
    elif mode == A_CONV3X3:
        c = s["conv"]
        F = M // (c["Hout"] * c["Wout"])
        band = _wide(g, data, F * c["Hin"] * c["Win"], c["Cin"]).reshape(-1) if wide else _rand(g, data, F * c["Hin"] * c["Win"] * c["Cin"])
        conv = dict(c)
        if s.get("x_halo"):
            off = (band.numel() + 15) // 16 * 16 + 64          # >= 64 poisoned elements between band and block, a multiple of 16
            a32 = torch.full((off + 2 * F * c["Hin"] * c["Cin"],), NAN)
            a32[: band.numel()] = band
            a32[off:] = _rand(g, data, 2 * F * c["Hin"] * c["Cin"])
            conv["x_halo_off"] = off
        else:
            a32 = band
        kw["conv"] = conv
    else:
        t = s["tconv"]
        rows = M + (2 * (M // (t["T"] * t["Npix"])) * t["Npix"] if t.get("halo") else 0)      # t_halo: T + 2 frames per sample
        a32 = _wide(g, data, rows, t["C"]).reshape(-1) if wide else _rand(g, data, rows * t["C"])
        kw["tconv"] = dict(t)
    hi, lo = split_planes(a32, s.get("a_lo"))
    planes = dict(a16=Plane(hi))
    if lo is not None:
        planes["a16_lo"] = Plane(lo)
        # (for the conditions of tests/test_gemm_range_ref64.py) the part of A's elements whose residual is beyond the e4m3 clamp
        planes["a16_lo"].clamped = (((a32 - hi.float()) * 2048.0).abs() > 448.0).sum().item() / (~torch.isnan(a32)).sum().item()
    # ---- W
    w_ld = s.get("w_ld", K + 8 if mode == A_PLAIN else K)
    w32 = _rand(g, data, N, K, scale=K ** -0.5, offset=0.0)
    if wide:
        w32 = w32 * 2.0 ** s["g"]
    if torch.is_tensor(pre_sc):
        w32 = w32 * pre_sc.view(N, 1)
    wh = w32.half()
    planes["w16"] = Plane(strided(wh, w_ld), (N, K) if w_ld == K else None)
    if w_ld != K:
        kw["w_ld"] = w_ld
    w_exp = None
    if s.get("a_lo") == "e4m3":
        w8, w_exp = engine.pk_lo8(wh)
        planes["w_lo"] = Plane(w8, (N, K))
    wl = strided(((w32 - wh.float()) * 2048.0).half(), w_ld)
    if s.get("w_split") == "w_lo":
        planes["w_lo"] = Plane(wl)
    elif s.get("w_split") == "w_lo16":
        planes["w_lo16"] = Plane(wl, (N, K) if w_ld == K else None)
    # ---- epilogue streams
    geglu = "geglu" in epi
    No = N // 2 if geglu else N
    vt = "vt" in epi
    ns = s["n_split"] if vt else No
    ldc32, ldc16 = s.get("ldc32", ns + 8), s.get("ldc16", ns + 8)
    if "bias" in epi:
        planes["bias"] = Plane(_rand(g, data, N) * (2.0 ** s["g"] if wide else pre_sc))      # (wide-rows: at the weights' scale)
    if "rb" in epi:
        kw.update(rb_rows=s["rb_rows"], rb_mod=s["rb_mod"])
        planes["rowbias"] = Plane(_rand(g, data, s["rb_mod"] * N).view(s["rb_mod"], N) * pre_sc)
    outs, alias = {}, {}
    r1 = None
    if "r1" in epi or "r1alias" in epi:
        kw["ldr1"] = ldc32 if "r1alias" in epi else s.get("ldr1", N + 4)
        r1 = strided(_rand(g, data, M, N) * out_sc, kw["ldr1"])
        if "r1" in epi:
            planes["res1"] = Plane(r1)
    if "r2" in epi:
        kw["ldr2"] = s.get("ldr2", N + 4)
        planes["res2"] = Plane(strided(_rand(g, data, M, N) * out_sc, kw["ldr2"]))
    if "silu" in epi:
        kw["act"] = ACT_SILU
    if "gelu" in epi:
        kw["act"] = ACT_GELU
    if geglu:
        kw["geglu"] = True
    # ---- outputs: poison everywhere (an aliased residual stream starts as the residual)
    if "o32" in epi:
        kw["ldc32"] = ldc32
        outs["out32"] = Plane(r1 if "r1alias" in epi else torch.full(((M - 1) * ldc32 + ns,), NAN))
        if "r1alias" in epi:
            alias["res1"] = "out32"
    if "o16" in epi:
        kw["ldc16"] = ldc16
        outs["out16"] = Plane(torch.full(((M - 1) * ldc16 + ns,), NAN, dtype=torch.float16))
        if "lo16" in epi:
            outs["out16_lo"] = Plane(torch.full(((M - 1) * ldc16 + ns,), NAN, dtype=torch.float16))
        if "lo8" in epi:
            outs["out16_lo"] = Plane(torch.full(((M - 1) * ldc16 + ns,), 0xFF, dtype=torch.uint8))
    if vt:
        t_rows, ldt = s["t_rows"], s["ldt"]
        gs = (No - ns) * ldt + 8
        kw.update(n_split=ns, t_rows=t_rows, ldt=ldt, t_gstride=gs)
        outs["out16t"] = Plane(torch.full(((M // t_rows - 1) * gs + (No - ns - 1) * ldt + t_rows,), NAN, dtype=torch.float16))
    return kw, planes, outs, alias, w_exp


# ----------------------------------------------------------------------------------------------------------------------- cases
def _plain_cases():
    out = []
    M, K = 300, 328
    tile_n = {1: 200, 2: 200, 3: 320, 4: 256}            # OPT_GEMM_TILE: 128x128, 256x128, 256x320, 256x256
    epis = ["o32", "bias+o32+o16+lo16", "bias+o32+o16+lo8", "bias+rb+r1alias+r2+o32", "bias+silu+o32+o16", "bias+gelu+o16+lo16"]
    for tile, N in tile_n.items():
        base = dict(mode=A_PLAIN, M=M, N=N, K=K, rb_rows=50, rb_mod=4, opts=dict(gemm_tile=tile))
        for e in epis:
            out.append(Case(f"plain-t{tile}-N{N}-{e}", "plain", dict(base, epi=e)))
        out.append(Case(f"plain-t{tile}-N{N}-alo16", "plain lo", dict(base, epi="bias+o32", a_lo="f16")))
        out.append(Case(f"plain-t{tile}-N{N}-alo8", "plain lo", dict(base, epi="bias+o32", a_lo="e4m3", K=336, lda=352, w_ld=336)))
        out.append(Case(f"plain-t{tile}-N{N}-alo16-wlo", "plain lo", dict(base, epi="o32", a_lo="f16", w_split="w_lo")))
        out.append(Case(f"plain-t{tile}-N{N}-wlo16", "plain lo", dict(base, epi="o32", w_split="w_lo16")))
        out.append(Case(f"plain-t{tile}-N{N}-alo8-wlo16", "plain lo",
                        dict(base, epi="o32", a_lo="e4m3", w_split="w_lo16", K=336, lda=352, w_ld=336)))
        out.append(Case(f"plain-t{tile}-N512-geglu", "plain", dict(base, N=512, epi="bias+geglu+o16+lo16")))
        # V^T: q | k row-major for n < 256, channel-major groups of t_rows = 80 rows behind (fast: every size a multiple of 8)
        out.append(Case(f"plain-t{tile}-N384-vt80", "plain", dict(base, M=320, N=384, epi="bias+o16+lo16+vt", n_split=256, t_rows=80, ldt=88)))
    base = dict(mode=A_PLAIN, M=M, K=K, rb_rows=50, rb_mod=4)
    out.append(Case("plain-N384-vt75-generic", "plain", dict(base, N=384, epi="bias+o16+lo16+vt", n_split=256, t_rows=75, ldt=78)))
    odd = dict(ldc32=105, ldc16=103, ldr1=101, ldr2=103)      # N = 100: N % 8 != 0 and odd leading dimensions -> E_GENERIC
    out.append(Case("plain-N100-generic-silu", "plain", dict(base, N=100, epi="bias+rb+r1+r2+silu+o32+o16+lo16", **odd)))
    out.append(Case("plain-N100-generic-gelu", "plain", dict(base, N=100, epi="bias+gelu+o32+o16+lo8", **odd)))
    for N in (16, 32):                                      # the 128x32 tile
        out.append(Case(f"plain-N{N}-narrow", "plain", dict(base, N=N, epi="bias+o32+o16+lo16")))
    return out


def _splitk_cases():
    return [Case("splitk-M300-N256-K3144", "split-K", dict(mode=A_PLAIN, M=300, N=256, K=3144, epi="bias+r1+o32+o16+lo16", splitk=True))]


def _conv_geo(kind, Hin, Win):
    if kind == "up":
        return dict(Hout=2 * Hin, Wout=2 * Win, stride=1, upsample=1)
    if kind == "padbr":                                      # F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2, padding 0)
        return dict(Hout=(Hin + 1 - 3) // 2 + 1, Wout=(Win + 1 - 3) // 2 + 1, stride=2, upsample=0, pad_br=1)
    st = 2 if kind == "s2" else 1
    return dict(Hout=(Hin + 2 - 3) // st + 1, Wout=(Win + 2 - 3) // st + 1, stride=st, upsample=0)


CONV_GEOS = [("s1", 9, 11, 0), ("s2", 9, 11, 0), ("s2", 8, 10, 0), ("padbr", 9, 11, 0), ("padbr", 8, 10, 0), ("up", 5, 7, 0),
             ("s1", 1, 40, 0), ("s1", 40, 1, 0), ("s1", 9, 11, 1), ("s2", 9, 11, 1), ("up", 5, 7, 1)]


def _conv3x3_cases():
    """per-tap kernels.  Every geometry at every Cin; N walks {8, 200, 320} so that every (geometry, N) and every (Cin, N) pair occurs.
    F: the smallest count for which M >= 290, so that 128- and 256-row tiles span frames; F = 2 with a column block."""
    out = []
    for gi, (kind, Hin, Win, halo) in enumerate(CONV_GEOS):
        for ci, Cin in enumerate((8, 24, 64, 128)):
            N = (8, 200, 320)[(gi + ci) % 3]
            geo = _conv_geo(kind, Hin, Win)
            F = 2 if halo else -(-290 // (geo["Hout"] * geo["Wout"]))
            conv = dict(Cin=Cin, Hin=Hin, Win=Win, **geo)
            out.append(Case(f"conv3x3-{kind}-{Hin}x{Win}{'-halo' if halo else ''}-C{Cin}-N{N}", "conv3x3 per-tap",
                            dict(mode=A_CONV3X3, M=F * geo["Hout"] * geo["Wout"], N=N, K=9 * Cin, conv=conv, x_halo=halo, epi="bias+o32",
                                 opts=dict(stencil_tiles=0))))
    return out


def _stencil_cases():
    out = []
    i = 0
    for H, W in ((16, 16), (8, 32)):
        for Cin in (64, 128):
            for N in (320, 192):
                spec = dict(mode=A_CONV3X3, M=3 * H * W, N=N, K=9 * Cin, conv=dict(Cin=Cin, Hin=H, Win=W, **_conv_geo("s1", H, W)),
                            epi=("bias+o32", "bias+r1alias+o32+o16")[i % 2], a_lo=(None, "f16")[(i // 2) % 2], ldc32=N, ldc16=N,
                            opts=dict(stencil_tiles=2), stencil=True)
                out.append(Case(f"stencil-{H}x{W}-C{Cin}-N{N}-{spec['epi']}{'-alo16' if spec['a_lo'] else ''}", "conv3x3 stencil", spec))
                i += 1
    for H, W, Cin, N, e, alo, extra, tag in ((16, 16, 64, 320, "bias+o32", None, dict(x_halo=1), "halo"),
                                             (8, 32, 128, 192, "bias+r1alias+o32+o16", "f16", dict(x_halo=1), "halo-alo16"),
                                             (16, 16, 128, 320, "bias+o32", None, dict(w_split="w_lo16"), "wlo16"),
                                             (8, 32, 64, 192, "bias+r1alias+o32+o16", None, dict(w_split="w_lo16"), "wlo16")):
        spec = dict(mode=A_CONV3X3, M=3 * H * W, N=N, K=9 * Cin, conv=dict(Cin=Cin, Hin=H, Win=W, **_conv_geo("s1", H, W)), epi=e, a_lo=alo,
                    ldc32=N, ldc16=N, opts=dict(stencil_tiles=2), stencil=True, **extra)
        out.append(Case(f"stencil-{H}x{W}-C{Cin}-N{N}-{e}-{tag}", "conv3x3 stencil", spec))
    return out


def _conv1d_cases():
    out = []
    B, Npix = 2, 50
    epis = ("bias+r1alias+rb+o32", "bias+r1+r2+o32+o16")
    i = 0
    for T in (1, 2, 3, 8, 9):
        for C in (24, 64, 128):
            base = dict(mode=A_CONV1D_T, M=B * T * Npix, N=C, K=3 * C, rb_rows=Npix, rb_mod=B * T, ldc32=C, ldc16=C, ldr1=C, ldr2=C)
            for e in epis:
                out.append(Case(f"conv1d-T{T}-C{C}-{e}", "conv1d", dict(base, tconv=dict(C=C, T=T, Npix=Npix), epi=e)))
            out.append(Case(f"conv1d-T{T}-C{C}-halo", "conv1d", dict(base, tconv=dict(C=C, T=T, Npix=Npix, halo=1), epi=epis[i % 2])))
            i += 1
        base = dict(mode=A_CONV1D_T, M=B * T * Npix, N=64, K=192, rb_rows=Npix, rb_mod=B * T, ldc32=64, ldc16=64, ldr1=64, ldr2=64)
        out.append(Case(f"conv1d-T{T}-C64-alo8{'-halo' if T in (2, 8) else ''}", "conv1d",
                        dict(base, tconv=dict(C=64, T=T, Npix=Npix, halo=int(T in (2, 8))), epi=epis[T % 2], a_lo="e4m3")))
    return out


CASES = _plain_cases() + _splitk_cases() + _conv3x3_cases() + _stencil_cases() + _conv1d_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# -------------------------------------------------------------------------------------------------------------- over the range
# The cases above are unit scale.  RANGE_CASES walk the NUMBER range on the same machinery (poisoned margins and gaps, NaN outputs):
#   wide-rows    the consumer side.  Storage row i of A lies in binade -24 + i % 38 (fp16 subnormals up to 2^13), graded by ROW so
#                that the lo pass of a row stays visible next to its hi pass; split_planes then writes e4m3 lo bytes from the
#                format's subnormals up to the +-448 of a clamped producer (|v| >= 512).  The weights are scaled by 2^g, g walking
#                G_WALK over the list: w_lo_exp from ~97 to ~130, fp16-subnormal weights at g = -20.  out32 only (results reach 1e7).
#                K = 48 is the sharp check of the lo pass (its 2^-12 mag against a bound of 2 K_passes u mag), K = 336 the loop + tail.
#   graded-cols  the producer side.  Unit-scale activations; row n of W, bias[n], the rowbias and the residual columns are scaled by
#                2^grade(n), linear from -24 to the case's top grade (Case.build: from the reference): outputs from fp16 subnormals
#                to beyond the e4m3 lo plane's clamp, pre-activations beyond +-88, GEGLU gates beyond +-8.
# spec["unit"]: what the range monitor counts for the case's writer (gemm_ref64.bound, point 7).
def _wide_cases():
    out = []
    tile_n = {1: 200, 2: 200, 3: 320, 4: 256}

    def add(name, family, spec):
        i = len(out)
        g = G_WALK[(i + i // 5) % 5]
        if g == -20 and spec["K"] == 48 and spec.get("a_lo") == "e4m3":
            # the sharp checks of the e4m3 lo pass need weights the MFMA's adder resolves: fp16-subnormal weights are aligned at 2^-14
            # (gemm_ref64.bound, point 8) and the lo pass is below that.  K = 336 and the conv gathers carry g = -20 for the pair
            g = 12
        out.append(Case(name, family, dict(spec, range="wide-rows", g=g)))

    for tile, N in tile_n.items():
        for K in (48, 336):
            base = dict(mode=A_PLAIN, M=300, N=N, K=K, lda=K + 16, w_ld=K, opts=dict(gemm_tile=tile))
            tag = f"wide-t{tile}-N{N}-K{K}"
            add(f"{tag}-alo8", "wide plain", dict(base, epi="bias+o32", a_lo="e4m3"))
            add(f"{tag}-alo8-wlo16", "wide plain", dict(base, epi="o32", a_lo="e4m3", w_split="w_lo16"))
            add(f"{tag}-alo16", "wide plain", dict(base, epi="bias+o32", a_lo="f16"))
            add(f"{tag}-alo16-wlo", "wide plain", dict(base, epi="o32", a_lo="f16", w_split="w_lo"))
            add(f"{tag}-wlo16", "wide plain", dict(base, epi="o32", w_split="w_lo16"))
    base = dict(mode=A_PLAIN, M=300)
    add("wide-N16-narrow-K48-alo8", "wide plain", dict(base, N=16, K=48, lda=64, w_ld=48, epi="o32", a_lo="e4m3"))
    add("wide-N32-narrow-K336-alo16", "wide plain", dict(base, N=32, K=336, lda=352, w_ld=336, epi="bias+o32", a_lo="f16"))
    for kind, Hin, Win in (("s1", 9, 11), ("up", 5, 7)):
        geo = _conv_geo(kind, Hin, Win)
        F = -(-290 // (geo["Hout"] * geo["Wout"]))
        add(f"wide-conv3x3-{kind}-{Hin}x{Win}-C64-N200-alo8", "wide conv",
            dict(mode=A_CONV3X3, M=F * geo["Hout"] * geo["Wout"], N=200, K=576, conv=dict(Cin=64, Hin=Hin, Win=Win, **geo), x_halo=0,
                 epi="bias+o32", a_lo="e4m3", opts=dict(stencil_tiles=0)))
    for T in (2, 9):
        for halo in (0, 1):
            add(f"wide-conv1d-T{T}-C64-alo8{'-halo' if halo else ''}", "wide conv",
                dict(mode=A_CONV1D_T, M=2 * T * 50, N=64, K=192, ldc32=64, tconv=dict(C=64, T=T, Npix=50, halo=halo), epi="bias+o32",
                     a_lo="e4m3"))
    add("wide-stencil-16x16-C64-N320-alo16", "wide conv",
        dict(mode=A_CONV3X3, M=3 * 256, N=320, K=576, conv=dict(Cin=64, Hin=16, Win=16, **_conv_geo("s1", 16, 16)), epi="bias+o32",
             a_lo="f16", ldc32=320, opts=dict(stencil_tiles=2), stencil=True))
    add("wide-splitk-M300-N256-K3152-alo8", "wide split-K",
        dict(mode=A_PLAIN, M=300, N=256, K=3152, lda=3168, w_ld=3152, epi="bias+o32", a_lo="e4m3", splitk=True))
    return out


def _graded_cases():
    out = []
    M, K = 300, 328
    tile_n = {1: 200, 2: 200, 3: 320, 4: 256}

    def add(name, family, spec, unit="quads"):
        out.append(Case(name, family, dict(spec, range="graded-cols", unit=unit, rb_rows=50, rb_mod=4)))

    for tile, N in tile_n.items():
        base = dict(mode=A_PLAIN, M=M, N=N, K=K, opts=dict(gemm_tile=tile))
        for e in ("bias+o32+o16+lo8", "bias+o32+o16+lo16"):
            add(f"graded-t{tile}-N{N}-{e}", "graded plain", dict(base, epi=e))
    t = {n: dict(mode=A_PLAIN, M=M, N=N, K=K, opts=dict(gemm_tile=n)) for n, N in tile_n.items()}
    add("graded-t1-N200-bias+silu+o32+o16", "graded act", dict(t[1], epi="bias+silu+o32+o16"))
    add("graded-t3-N320-bias+silu+o32+o16", "graded act", dict(t[3], epi="bias+silu+o32+o16"))
    # GELU next to an out32 has no specialised variant (select_epilogue): the generic epilogue, which counts elements
    add("graded-t2-N200-bias+gelu+o32+o16+lo8", "graded act", dict(t[2], epi="bias+gelu+o32+o16+lo8"), unit="elements")
    add("graded-t4-N256-bias+gelu+o16+lo16", "graded act", dict(t[4], epi="bias+gelu+o16+lo16"))
    add("graded-t1-N200-bias+gelu+o16+lo16", "graded act", dict(t[1], epi="bias+gelu+o16+lo16"))
    add("graded-t3-N512-geglu", "graded act", dict(t[3], N=512, epi="bias+geglu+o16+lo16"))
    add("graded-t2-N384-vt80", "graded plain", dict(t[2], M=320, N=384, epi="bias+o16+lo16+vt", n_split=256, t_rows=80, ldt=88))
    base = dict(mode=A_PLAIN, M=M, K=K)
    odd = dict(ldc32=105, ldc16=103, ldr1=101, ldr2=103)      # N % 8 != 0, odd leading dimensions: the generic epilogue
    add("graded-N100-generic-silu", "graded act", dict(base, N=100, epi="bias+rb+r1+r2+silu+o32+o16+lo16", **odd), unit="elements")
    add("graded-N100-generic-gelu", "graded act", dict(base, N=100, epi="bias+gelu+o32+o16+lo8", **odd), unit="elements")
    # the 128x32 tile has two fast epilogues, out32 alone and out16 alone (gemm_dispatch.h): both outputs go through the generic one
    add("graded-N16-narrow", "graded plain", dict(base, N=16, epi="bias+o32+o16+lo8"), unit="elements")
    for lo in ("lo16", "lo8"):
        add(f"graded-splitk-M300-N256-K3144-{lo}", "graded split-K",
            dict(mode=A_PLAIN, M=300, N=256, K=3144, epi=f"bias+r1+o32+o16+{lo}", splitk=True))
    add("graded-conv1d-T3-C64-bias+r1+r2+o32+o16", "graded conv",
        dict(mode=A_CONV1D_T, M=300, N=64, K=192, ldc32=64, ldc16=64, ldr1=64, ldr2=64, tconv=dict(C=64, T=3, Npix=50),
             epi="bias+r1+r2+o32+o16"))
    add("graded-stencil-16x16-C64-N320-bias+r1alias+o32+o16", "graded conv",
        dict(mode=A_CONV3X3, M=3 * 256, N=320, K=576, conv=dict(Cin=64, Hin=16, Win=16, **_conv_geo("s1", 16, 16)),
             epi="bias+r1alias+o32+o16", ldc32=320, ldc16=320, opts=dict(stencil_tiles=2), stencil=True))
    # no out32: the planes and the monitor are held to the reference alone.  K = 72 and positive data keep 2^11 b small against 448
    add("graded-t1-N200-K72-o16+lo8", "graded plain", dict(t[1], K=72, epi="o16+lo8", only="graded-cols+"))
    return out


RANGE_CASES = _wide_cases() + _graded_cases()
RANGE_BY_NAME = {c.name: c for c in RANGE_CASES}
assert len(RANGE_BY_NAME) == len(RANGE_CASES) and not set(RANGE_BY_NAME) & set(BY_NAME)
# one launch each: a case on the two variants of its family (a case with `only`: on that one)
RANGE_RUNS = [(c, d) for c in RANGE_CASES for d in RANGE_DATA if d.startswith(c.spec["range"]) and c.spec.get("only", d) == d]
RANGE_IDS = [f"{c.name}-{d}" for c, d in RANGE_RUNS]


# ------------------------------------------------------------------------------------------------------------------- the checks
_REF = {}


def reference(case, data):
    """the float64 expectation of a case, computed once from the CPU operands, shared by the tests and left unchanged"""
    if (case.name, data) not in _REF:
        _REF[case.name, data] = gemm_ref64.gemm(**case.launch(data)[0])
    return _REF[case.name, data]


def lo_values(t):
    return t.view(torch.float8_e4m3fn).float() if t.dtype == torch.uint8 else t.float()


def check_outputs(case, data, r, bound, kw, allocs):
    """What every launch of a case has to satisfy, for the tensors `kw` / `allocs` of Case.launch after the launch (any device):
    every element gemm_ref64 marks as written is finite and within `bound` of the float64 value (lo planes: the reconstructed
    hi + 2^-11 lo), every other element of every output allocation — leading-dimension gaps, rows past M, margins — holds the bits
    it started with.  -> {output: worst err / bound}; raises AssertionError naming the case, the first bad index and err / bound."""
    tag = f"{case.name} [{data}]"
    worst = {}
    start = case.build(data)[2]
    for name, (idx, cols) in r["outs"].items():
        flat = kw["out16" if name == "out16_lo" else name].reshape(-1).cpu()
        got = flat.double()[idx]
        if name == "out16_lo":
            got = got + lo_values(kw[name].reshape(-1).cpu()).double()[idx] * 2.0 ** -11
        ref, b = r["v"][:, cols], bound(r, name)
        bad = ~torch.isfinite(got)
        assert not bad.any(), f"{tag} {name}: {int(bad.sum())} of {got.numel()} written elements are not finite, first (m, n) = " \
                              f"{torch.nonzero(bad)[0].tolist()}"
        ratio = (got - ref).abs() / b
        worst[name] = ratio.max().item()
        if worst[name] > 1.0:
            m, n = torch.nonzero(ratio > 1.0)[0].tolist()
            raise AssertionError(f"{tag} {name}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements outside the bound, worst err / bound "
                                 f"{worst[name]:.3g}; first bad (m, n) = ({m}, {n}): got {got[m, n].item():.9g}, float64 {ref[m, n].item():.9g}, "
                                 f"bound {b[m, n].item():.3g}")
    for name, alloc in allocs.items():
        written = torch.zeros(alloc.numel(), dtype=torch.bool)
        written[MARGIN + r["outs"][name][0].reshape(-1)] = True
        bits = torch.uint8 if alloc.dtype == torch.uint8 else torch.int32 if alloc.dtype == torch.float32 else torch.int16
        now, was = alloc.cpu().view(bits), start[name].alloc.view(bits)
        touched = (now != was) & ~written
        assert not touched.any(), f"{tag} {name}: {int(touched.sum())} elements outside the written set changed, first at element " \
                                  f"{int(torch.nonzero(touched)[0]) - MARGIN} of the view"
    return worst


def check_range(case, data, r, kw, count):
    """What a launch of a RANGE case has to satisfy beyond check_outputs (gemm_ref64.bound, points 6 and 7), for the tensors `kw` of
    Case.launch after the launch and the range monitor's `count` over that one launch (None: not collected).  Which statement applies
    to an element is decided by the reference `r` and the case, never by the output."""
    tag = f"{case.name} [{data}]"
    outs = r["outs"]

    def written(name):
        return kw[name].reshape(-1).cpu()[outs[name][0]]

    expect = 0                                                  # nothing but an e4m3 out16_lo is counted
    if "out16_lo" in outs and r["out_lo_e4m3"]:
        lo, hi = written("out16_lo"), written("out16")
        nan = (lo & 0x7F) == 0x7F
        assert not nan.any(), f"{tag} out16_lo: {int(nan.sum())} written bytes are the e4m3 NaN code, first (m, n) = {torch.nonzero(nan)[0].tolist()}"
        unit = case.spec["unit"]
        if "out32" in outs:
            o32 = written("out32")
            bad = hi.view(torch.int16) != o32.half().view(torch.int16)
            assert not bad.any(), f"{tag} out16: {int(bad.sum())} elements are not fp16(out32), first (m, n) = {torch.nonzero(bad)[0].tolist()}"
            q, _ = misc_ref64.lo_e4m3(o32, hi)
            bad = lo_values(lo) != lo_values(q)
            if bad.any():
                m, n = torch.nonzero(bad)[0].tolist()
                raise AssertionError(f"{tag} out16_lo: {int(bad.sum())} bytes are not e4m3(clamp((out32 - out16) 2^11)), first (m, n) = "
                                     f"({m}, {n}): out32 {o32[m, n].item():.9g}, out16 {hi[m, n].item():.9g}, byte {int(lo[m, n]):#x}, "
                                     f"expected {int(q[m, n]):#x}")
            expect = gemm_ref64.monitor_expect(o32, hi, unit)
        else:
            expect = gemm_ref64.monitor_bracket(r, unit)
    if count is not None:
        if isinstance(expect, tuple):
            assert expect[0] <= count <= expect[1], f"{tag}: the range monitor counted {count} {unit}, the reference brackets {expect}"
        else:
            assert count == expect, f"{tag}: the range monitor counted {count}, the launch's own out32 implies {expect} " \
                                    f"{case.spec.get('unit', 'quads')}"
    tail = gemm_ref64.silu_tail(r)
    if tail is not None:
        for name, (idx, cols) in outs.items():
            if name != "out16_lo":
                big = tail[:, cols] & ~(written(name).double().abs() < 2.0 ** -120)       # (a NaN is not below)
                assert not big.any(), f"{tag} {name}: SiLU of a pre-activation below -88 is neither 0 nor below 2^-120 at (m, n) = " \
                                      f"{torch.nonzero(big)[0].tolist()}"
    return expect
