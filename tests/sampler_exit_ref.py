"""Per-op fp32 reference of the sampler exit kernel (pnc_cfg_euler_step[_skip], pnc_cfg_sampler_step[_skip]), written from the
comment blocks of include/panacea_hip.h alone: it imports neither tests/emu.py nor panacea_amd.sampling.

`exit_step` evaluates one launch with torch fp32 CPU tensors, ONE elementwise torch op per rounding, in the header's order: real
fp32 + - * / (never float64 followed by a rounding: a division rounded twice is not the division rounded once).  Operands are
indexed from their flat storage with the header's layouts — eps tokens [(cfg ? 2 : 1) * T * Npix][ld] uncond half first, planes
NCHW [T][C][Npix], per-frame vectors [T] — one "thread" i = frame * Npix + pixel as the header's per-frame scalars imply.

The same function is two more things:
  * `mutant=NAME`: a WRONG kernel, the reference with one deviation (MUTANTS).  tests/test_sampler_exit_ref.py shows that every one
    of them leaves the reference's bits on the cases of tests/sampler_exit_cases.py, and a failing GPU comparison names the mutant, if
    any, whose bits the kernel has.
  * `tracked=True`: the formula in float64 with a running first-order error bound of the fp32 evaluation (class Tracked), the
    sanity check of the reference itself."""
import torch

HEUN1, HEUN2, EULER_A, DPM2S_1, DPM2S_2, DPM2M, LMS = range(7)          # PNC_SAMPLER_*
MODE_NAMES = ["HEUN1", "HEUN2", "EULER_A", "DPM2S_1", "DPM2S_2", "DPM2M", "LMS"]
N_VECTORS = {HEUN1: 2, HEUN2: 2, EULER_A: 4, DPM2S_1: 4, DPM2S_2: 5, DPM2M: 5}     # LMS: 2 + n_hist; DPM2M without aux: 2
WRITES_AUX = (HEUN1, DPM2S_1, DPM2M, LMS)

U32 = 2.0 ** -24            # unit roundoff of fp32, round to nearest

# name -> the one deviation from the header
MUTANTS = {
    "fma_all": "every a * b + c contracted into one rounding (float64, then rounded)",
    "fma_denoised": "contraction in the guided D only",
    "fma_update": "contraction in the mode's update only",
    "halves_swapped": "the cond half read first, the uncond half second",
    "cond_at_C": "the cond half read at element offset T * Npix * C instead of T * Npix * ld",
    "frame_npix_plus_1": "the frame of thread i taken as i / (Npix + 1)",
    "select_ge": "selectors v >= 0 instead of v > 0",
    "select_nan_true": "selectors !(v <= 0): a NaN selects",
    "select_sigma_up": "EULER_A / DPM2S_2: the noise term selected on sigma_up instead of next_sigma",
    "noise_assoc": "noise * (s_noise * sigma_up) instead of (noise * s_noise) * sigma_up",
    "lms_oldest_first": "LMS: coeff_k applied to the history planes oldest first",
    "lms_sum_reversed": "LMS: the history terms added oldest first (pairs kept)",
    "lms_no_zero_start": "LMS: the sum started from coeff_0 * d, a -0.0 kept, instead of 0 + coeff_0 * d",
    "dpm2m_aux_clobbered": "DPM2M with out_aux == aux: out_aux = D written before aux is read",
    "heun2_select_sigma_hat": "HEUN2 selecting on sigma_hat instead of next_sigma",
    "skip_adds_x": "skip path: D_h = eps * c_out + x instead of + x * c_skip",
}
_FMA_D = ("fma_all", "fma_denoised")
_FMA_U = ("fma_all", "fma_update")


class Tracked:
    """a float64 value with a bound `err` on |fp32 evaluation - value|, carried through + - * / by the standard model
    fl(a op b) = (a op b)(1 + delta), |delta| <= 2^-24: the operands' errors propagated to first order plus their product,
    plus one rounding of the result's magnitude.  Inputs are exact (err 0)."""

    def __init__(self, val, err=None):
        self.val = val.double() if torch.is_tensor(val) else torch.tensor(float(val), dtype=torch.float64)
        self.err = torch.zeros_like(self.val) if err is None else err

    @staticmethod
    def of(o):
        return o if isinstance(o, Tracked) else Tracked(o)

    def _rounded(self, val, err):
        return Tracked(val, err + U32 * (val.abs() + err))

    def __add__(self, o):
        o = Tracked.of(o)
        return self._rounded(self.val + o.val, self.err + o.err)

    __radd__ = __add__

    def __sub__(self, o):
        o = Tracked.of(o)
        return self._rounded(self.val - o.val, self.err + o.err)

    def __mul__(self, o):
        o = Tracked.of(o)
        return self._rounded(self.val * o.val, self.val.abs() * o.err + o.val.abs() * self.err + self.err * o.err)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Tracked.of(o)
        q = self.val / o.val
        return self._rounded(q, (self.err + q.abs() * o.err) / (o.val.abs() - o.err).clamp_min(0.0))


def _where(cond, a, b):
    if isinstance(a, Tracked) or isinstance(b, Tracked):
        a, b = Tracked.of(a), Tracked.of(b)
        return Tracked(torch.where(cond, a.val, b.val), torch.where(cond, a.err, b.err))
    return torch.where(cond, a, b)


def _fma(a, b, c):
    """a * b + c with ONE rounding: the product of two fp32 values is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def exit_step(mode, ops, shape, cfg, scale, s_noise=1.0, mutant=None, out_aux_is_aux=False, tracked=False):
    """-> (out, out_aux or None), [T, C, Npix] fp32 (tracked: Tracked).  `ops`: eps (flat tokens), x, c_out, v (list of [T]), and
    where the mode reads them c_skip, x0, aux, noise, hist (list, newest first); a missing c_skip is the eps path, a missing aux of
    DPM2M the first / last step.  `shape` = (T, C, Npix, ld).  `out_aux_is_aux`: the launch aliases out_aux and aux (only the
    mutant that gets the order wrong cares)."""
    assert mutant is None or (mutant in MUTANTS and not tracked)
    T, C, Npix, ld = shape
    f32 = torch.float32
    W = Tracked if tracked else (lambda t: t)
    thread = torch.arange(T * Npix).view(T, 1, Npix)
    frame = thread // (Npix + 1 if mutant == "frame_npix_plus_1" else Npix)
    raw = lambda vec: vec.reshape(-1)[frame]                                    # noqa: E731  [T, 1, Npix], the thread's frame scalar
    plane = lambda t: W(t.reshape(-1)[: T * C * Npix].view(T, C, Npix))       # noqa: E731

    def mac(a, b, c, fused):                                                    # a * b + c
        if fused:
            return _fma(*torch.broadcast_tensors(a, b, c))
        p = a * b
        return p + c

    def msub(a, b, c, fused):                                                   # a * b - c
        if fused:
            return _fma(*torch.broadcast_tensors(a, b, -c))
        p = a * b
        return p - c

    # ---- the guided denoised D
    eps = ops["eps"].reshape(-1)
    col = torch.arange(C).view(1, C, 1)
    cond0 = (T * Npix * (C if mutant == "cond_at_C" else ld)) if cfg else 0
    eu, ec = W(eps[thread * ld + col]), W(eps[cond0 + thread * ld + col])
    if mutant == "halves_swapped":
        eu, ec = ec, eu
    X = plane(ops["x"])
    co = W(raw(ops["c_out"]))
    xs = X
    if ops.get("c_skip") is not None and mutant != "skip_adds_x":
        xs = X * W(raw(ops["c_skip"]))
    fd, fu = mutant in _FMA_D, mutant in _FMA_U
    D = mac(ec, co, xs, fd)
    if cfg:
        Du = mac(eu, co, xs, fd)
        D = mac(W(torch.tensor(scale, dtype=f32)), D - Du, Du, fd)

    # ---- the mode's update
    vr = [raw(t) for t in ops["v"]]
    v = [W(t) for t in vr]

    def sel(k):
        if mutant == "select_ge":
            return vr[k] >= 0
        if mutant == "select_nan_true":
            return ~(vr[k] <= 0)
        return vr[k] > 0

    def noise_term(k_up):
        n, s = plane(ops["noise"]), W(torch.tensor(s_noise, dtype=f32))
        if mutant == "noise_assoc":
            return n, s * v[k_up]
        return n * s, v[k_up]

    def euler(k_sigma, k_next):                                                 # (d, x + (next - sigma) * d)
        d = (X - D) / v[k_sigma]
        return d, mac(v[k_next] - v[k_sigma], d, X, fu)

    out_aux = None
    if mode == HEUN1:
        out_aux, out = euler(0, 1)
    elif mode == HEUN2:
        d_new = (X - D) / v[1]
        d_prime = (plane(ops["aux"]) + d_new) / 2.0
        xc = mac(d_prime, v[1] - v[0], plane(ops["x0"]), fu)
        out = _where(sel(0 if mutant == "heun2_select_sigma_hat" else 1), xc, X)
    elif mode == EULER_A:
        _, y = euler(0, 1)
        out = _where(sel(2 if mutant == "select_sigma_up" else 3), mac(*noise_term(2), y, fu), y)
    elif mode == DPM2S_1:
        _, out_aux = euler(0, 1)
        out = msub(v[2], X, v[3] * D, fu)
    elif mode == DPM2S_2:
        y = _where(sel(2), msub(v[0], plane(ops["x0"]), v[1] * D, fu), plane(ops["aux"]))
        out = _where(sel(3 if mutant == "select_sigma_up" else 4), mac(*noise_term(3), y, fu), y)
    elif mode == DPM2M:
        out = msub(v[0], X, v[1] * D, fu)
        if ops.get("aux") is not None:
            old = D if (mutant == "dpm2m_aux_clobbered" and out_aux_is_aux) else plane(ops["aux"])
            dd = msub(v[2], D, v[3] * old, fu)
            out = _where(sel(4), msub(v[0], X, v[1] * dd, fu), out)
        out_aux = D
    elif mode == LMS:
        d = (X - D) / v[0]
        hist = [plane(h) for h in ops.get("hist", ())]
        terms = list(zip(v[2:2 + len(hist)], hist[::-1] if mutant == "lms_oldest_first" else hist))
        if mutant == "lms_sum_reversed":
            terms = terms[::-1]
        acc = v[1] * d
        if mutant != "lms_no_zero_start":
            acc = 0 + acc                                                        # sum() starts from the int 0: -0.0 becomes +0.0
        for coeff, h in terms:
            acc = mac(coeff, h, acc, fu)
        out = X + acc
        out_aux = d
    else:
        raise ValueError(f"mode {mode}")
    if not tracked:
        out = out.expand(T, C, Npix).contiguous()
        out_aux = None if out_aux is None else out_aux.expand(T, C, Npix).contiguous()
    return out, out_aux


# roundings on the longest path from an operand to `out`, per mode, with cfg and the skip term (the count the bound of
# Tracked accumulates along that path; tests/test_sampler_exit_ref.py prints it next to the bound it derives):
#   D: x * c_skip, eps * c_out, + ; the same for the other half in parallel; D_c - D_u, scale *, D_u +          = 6
ROUNDINGS_D = 6
ROUNDINGS_UPDATE = {HEUN1: 4,        # x - D, / sigma, dt * d (dt: one rounding in parallel), x +
                    HEUN2: 6,        # x - D, / next, aux +, / 2, * dt, x0 +
                    EULER_A: 5,      # HEUN1's four, + the noise term
                    DPM2S_1: 2,      # mult2 * D, mult1 x -          (out_aux: HEUN1's four)
                    DPM2S_2: 3,      # mult4 * D, mult3 x0 -, + the noise term
                    DPM2M: 4,        # mult3 * D, - mult4 aux, mult2 *, mult1 x -
                    LMS: 8}          # x - D, / sigma, coeff_0 *, 0 +, three history sums, x +
