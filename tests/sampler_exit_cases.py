"""Cases of the sampler exit kernel's bit-level tests (tests/test_sampler_exit_ref.py on the CPU, tests/test_sampler_exit_gpu.py on the
MI355X): every mode, entry and optional operand of pnc_cfg_sampler_step[_skip] / pnc_cfg_euler_step[_skip] at the shapes where the
indexing can go wrong, in poisoned allocations, with ONE launcher for panacea_amd.hip and tests/emu.py.

Shapes (T, C, Npix, ld) — one thread per (frame, pixel), 256 threads per workgroup:
  (1, 1, 1, 1)     one live thread
  (3, 4, 100, 8)   frame boundaries inside a workgroup, a partial last workgroup, padded token rows
  (2, 3, 257, 5)   odd C and ld, a frame that crosses a workgroup boundary by one thread
  (5, 4, 64, 4)    ld == C, more than four frames in one workgroup

Families:
  grid-MODE      mode x cfg {1, 0} x {eps entry, skip entry with c_skip = 0.3 + 0.17 frame} x the four shapes (LMS: three history
                 planes; DPM2M: with aux)
  lms-hist       LMS with 0, 1, 2, 3 history planes          dpm2m-noaux   DPM2M without aux (first / last step)
  scale          every mode at scale 5, 1, 0, -1.5           s_noise       EULER_A / DPM2S_2 at s_noise 0.9, 1, 0
  euler          the two Euler entries (the reference's HEUN1 `out`)
  unused         every operand the mode does not read passed as a fully poisoned plane / vector (the grid passes None)
  alias-MODE     the aliased launches the header allows: out / out_aux IS x0 / aux / hist[k]
  lms-negzero    one element whose coeff_0 * d is -0.0 and whose x is -0.0: `0 +` shows in the sign of out

Selectors.  At T >= 3 every selecting vector — HEUN2 v[1]; EULER_A v[3]; DPM2S_2 v[2] and v[4], independently; DPM2M v[4] — holds
positive frames and frames from {0.0, -0.0, negative} in ONE launch (T = 3: one non-positive frame, its kind rotating with the case;
T = 5: all three kinds), so both sides of every `v > 0 ? a : b` are taken inside one workgroup; HEUN2's deselected frames divide by
their zero.  The pure selectors (EULER_A v[3], DPM2S_2 v[4], DPM2M v[4]) hold a NaN frame at T = 5.  Divisors of selected paths
and every other per-frame vector are in [0.5, 1.5) (c_out negated, LMS coefficients with alternating signs).

Allocations.  Every operand and output is a view inside [MARGIN poison | body | MARGIN poison] (Data); the poison is a NaN with a
payload.  The eps body is the (cfg ? 2 : 1) * T * Npix rows of ld floats the header names: columns C .. ld - 1 are poison, and
what follows the last row is the margin — with cfg = 0 there is no second half to read.  Outputs start as poison (aliased: as the
operand they are).  `check` compares WHOLE allocations as int32, outputs, operands and margins alike."""
import dataclasses
import zlib

import torch

import sampler_exit_ref as ref
from sampler_exit_ref import DPM2M, DPM2S_1, DPM2S_2, EULER_A, HEUN1, HEUN2, LMS, MODE_NAMES

MARGIN = 64
POISON_BITS = 0x7FC5A5A5             # a quiet NaN with a payload
OTHER_POISON_BITS = 0x7F7FFFFF       # the largest finite fp32: a reference that read it would show it
SHAPES = [(1, 1, 1, 1), (3, 4, 100, 8), (2, 3, 257, 5), (5, 4, 64, 4)]
S1 = SHAPES[1]
NONPOS = [0.0, -0.0, -0.7]
NAN = float("nan")
PLANES = ("x0", "aux", "noise", "hist0", "hist1", "hist2")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str
    mode: int
    shape: tuple = S1
    cfg: int = 1
    skip: bool = False
    scale: float = 5.0
    s_noise: float = 0.9
    n_hist: int = 3                  # LMS
    with_aux: bool = True            # DPM2M
    z: int = 0                       # which of NONPOS the non-positive selector frame of a T = 3 launch holds
    alias: tuple = ()                # ((output, operand it IS), ...)
    unused_poison: bool = False
    entry: str = "struct"            # "euler": pnc_cfg_euler_step[_skip]
    special: str = ""                # "negzero"
    seed: int = 0                    # (raise to re-seed a case whose reference is not finite)

    def __repr__(self):
        return self.name

    @property
    def data_key(self):
        """what the operands' values depend on: cases that differ in aliasing, unused operands, scale or s_noise share them"""
        return (self.mode, self.shape, self.cfg, self.skip, self.n_hist if self.mode == LMS else 0, self.z, self.special, self.seed)

    @property
    def nv(self):
        """per-frame vectors the mode reads"""
        if self.mode == LMS:
            return 2 + self.n_hist
        return 2 if self.mode == DPM2M and not self.with_aux else ref.N_VECTORS[self.mode]

    @property
    def reads(self):
        """optional planes the mode reads"""
        return {HEUN1: (), HEUN2: ("x0", "aux"), EULER_A: ("noise",), DPM2S_1: (), DPM2S_2: ("x0", "aux", "noise"),
                DPM2M: ("aux",) if self.with_aux else (), LMS: tuple(f"hist{k}" for k in range(self.n_hist))}[self.mode]

    @property
    def writes_aux(self):
        return self.mode in ref.WRITES_AUX and self.entry == "struct"

    def unaliased(self):
        return dataclasses.replace(self, alias=(), name=self.name + "-unaliased")


class Data:
    """allocations {name: 1-D fp32 tensor} and the operands' places in them {operand: (allocation, first element, elements)}"""

    def __init__(self, allocs, span):
        self.allocs, self.span = allocs, span

    def view(self, name):
        if name not in self.span:
            return None
        a, start, n = self.span[name]
        return self.allocs[a][start:start + n]

    def to(self, device):
        return Data({n: a.clone().to(device) for n, a in self.allocs.items()}, self.span)

    def cpu(self):
        return Data({n: a.cpu() for n, a in self.allocs.items()}, self.span)


def bits(t):
    return t.view(torch.int32)


def _poisoned(n, poison_bits):
    return torch.full((n,), poison_bits, dtype=torch.int32).view(torch.float32)


def _selectors(case, T, pos):
    """{vector index: [T] values} of the mode's selecting vectors; `pos()` draws a positive [T] vector"""
    if T < 3:
        return {}
    n = lambda k: NONPOS[(case.z + k) % 3]                                                # noqa: E731
    mixed = {3: [1, n(0), 1], 5: [1, 0.0, 1, -0.0, -0.7]}[T]
    pure = {3: [1, n(0), 1], 5: [1, 0.0, NAN, -0.0, -0.7]}[T]
    second = {3: [1, 1, n(1)], 5: [1, 1, NAN, -0.0, -1.3]}[T]                              # DPM2S_2 v[4] next to v[2] = first
    first = {3: [1, n(0), 1], 5: [1, 0.0, 1, -0.7, 1]}[T]
    pick = {HEUN2: {1: mixed}, EULER_A: {3: pure}, DPM2S_2: {2: first, 4: second}, DPM2M: {4: pure} if case.with_aux else {}}
    out = {}
    for k, pattern in pick.get(case.mode, {}).items():
        p = pos()
        out[k] = torch.where(torch.tensor(pattern) == 1, p, torch.tensor(pattern, dtype=torch.float32))
    return out


_BUILT = {}


def build(case, poison_bits=POISON_BITS):
    """the launch's allocations on the CPU as they are BEFORE the launch (cached; never modified: `.to()` copies)"""
    key = (case, poison_bits)
    if key in _BUILT:
        return _BUILT[key]
    T, C, Npix, ld = case.shape
    g = torch.Generator().manual_seed(zlib.crc32(repr(case.data_key).encode()) % (2 ** 31))
    randn = lambda *s: torch.randn(*s, generator=g)                                       # noqa: E731
    pos = lambda: torch.rand(T, generator=g) + 0.5                                        # noqa: E731
    # every draw happens for every case, in one order: cases with the same data_key share every value
    rows = (2 if case.cfg else 1) * T * Npix
    tok = _poisoned(rows * ld, poison_bits).view(rows, ld)
    tok[:, :C] = randn(rows, C)
    body = {"eps": tok.reshape(-1), "x": randn(T * C * Npix)}
    for name in PLANES:
        body[name] = randn(T * C * Npix)
    body["c_out"] = -pos()
    body["c_skip"] = torch.arange(T, dtype=torch.float32) * 0.17 + 0.3
    v = [pos() for _ in range(6)]
    if case.mode == LMS:
        for k in range(1, 6):
            v[k] = v[k] * (-1.0) ** (k - 1)
    for k, vec in _selectors(case, T, pos).items():
        v[k] = vec
    if case.special == "negzero":            # thread 0, channel 0: eps = 0 in both halves, x = -0.0, and the sign of coeff_0 that
        body["x"][0] = -0.0                   # makes coeff_0 * d a -0.0 (cfg: d = -0.0; no cfg: d = +0.0)
        tok[0, 0] = 0.0
        tok[rows // 2 if case.cfg else 0, 0] = 0.0
        v[1][0] = v[1][0].abs() * (1.0 if case.cfg else -1.0)
    for k in range(6):
        body[f"v{k}"] = v[k]

    present = {"eps", "x", "c_out"} | {f"v{k}" for k in range(case.nv)} | set(case.reads)
    if case.skip:
        present.add("c_skip")
    if case.unused_poison:                    # what the mode does not read: poison all through
        unused = [f"v{k}" for k in range(case.nv, 6)]
        if case.entry == "struct":
            unused += [p for p in PLANES if p not in case.reads and not (p == "aux" and case.mode == DPM2M)]
            if case.mode == LMS:              # (the planes beyond n_hist would be n_hist itself)
                unused = [u for u in unused if not u.startswith("hist")]
        for name in unused:
            body[name] = _poisoned(body[name].numel(), poison_bits)
        present |= set(unused)
    allocs, span = {}, {}
    for name in sorted(present):
        n = body[name].numel()
        allocs[name] = _poisoned(n + 2 * MARGIN, poison_bits)
        allocs[name][MARGIN:MARGIN + n] = body[name]
        span[name] = (name, MARGIN, n)
    outs = ["out"] + (["out_aux"] if case.writes_aux or (case.unused_poison and case.entry == "struct") else [])
    for name in outs:
        target = dict(case.alias).get(name)
        if target:
            assert target in case.reads, (case.name, target)
            span[name] = span[target]
        else:
            allocs[name] = _poisoned(T * C * Npix + 2 * MARGIN, poison_bits)
            span[name] = (name, MARGIN, T * C * Npix)
    _BUILT[key] = Data(allocs, span)
    return _BUILT[key]


def operands(case, data):
    """the `ops` of sampler_exit_ref.exit_step: the operands the mode reads"""
    ops = {n: data.view(n) for n in ("eps", "x", "c_out") + tuple(r for r in case.reads if not r.startswith("hist"))}
    ops["v"] = [data.view(f"v{k}") for k in range(case.nv)]
    ops["hist"] = [data.view(r) for r in case.reads if r.startswith("hist")]
    if case.skip:
        ops["c_skip"] = data.view("c_skip")
    return ops


def outputs(case, data, mutant=None, tracked=False):
    """(out, out_aux or None) of the reference (or of a wrong-kernel model) on the operands in `data`"""
    out, out_aux = ref.exit_step(case.mode, operands(case, data), case.shape, case.cfg, case.scale, case.s_noise, mutant=mutant,
                                 out_aux_is_aux=dict(case.alias).get("out_aux") == "aux", tracked=tracked)
    return out, (out_aux if case.writes_aux else None)


_WANT = {}


def reference(case, poison_bits=POISON_BITS, mutant=None):
    """the allocations as they must be AFTER the launch (cached for the reference, computed once and left unchanged)"""
    key = (case, poison_bits)
    if mutant is None and key in _WANT:
        return _WANT[key]
    want = build(case, poison_bits).to("cpu")
    out, out_aux = outputs(case, want, mutant)            # both computed before either is written: the launch's contract
    want.view("out").copy_(out.reshape(-1))
    if out_aux is not None:
        want.view("out_aux").copy_(out_aux.reshape(-1))
    if mutant is None:
        _WANT[key] = want
    return want


def launch(mod, case, data):
    """the case through mod.cfg_sampler_step / mod.cfg_euler_step (mod: panacea_amd.hip or tests/emu.py) on the tensors of `data`,
    which the launch modifies"""
    T, C, Npix, ld = case.shape
    v = [data.view(f"v{k}") for k in range(6) if f"v{k}" in data.span]
    if case.entry == "euler":
        mod.cfg_euler_step(data.view("eps"), ld, T, Npix, C, case.cfg, case.scale, data.view("x"), data.view("c_out"), v[0], v[1],
                           data.view("out"), c_skip=data.view("c_skip"))
        return
    hist = [data.view(f"hist{k}") for k in range(3) if f"hist{k}" in data.span]
    mod.cfg_sampler_step(case.mode, data.view("eps"), ld, T, Npix, C, case.cfg, case.scale, data.view("x"), data.view("c_out"), v,
                         data.view("out"), out_aux=data.view("out_aux"), x0=data.view("x0"), aux=data.view("aux"), hist=hist,
                         noise=data.view("noise"), s_noise=case.s_noise, c_skip=data.view("c_skip"))


def differing(got, want):
    """{allocation: bool mask of the elements whose bits differ}"""
    assert set(got.allocs) == set(want.allocs)
    return {n: bits(got.allocs[n].cpu()) != bits(want.allocs[n]) for n in want.allocs}


def count(case, got, want):
    """(elements compared in the output planes, elements of any allocation that differ)"""
    T, C, Npix, _ = case.shape
    return T * C * Npix * (2 if case.writes_aux else 1), sum(int(m.sum()) for m in differing(got, want).values())


def _hex(t):
    return f"0x{int(bits(t.reshape(1))[0]) & 0xFFFFFFFF:08X}"


def matching_mutants(case, got):
    """the wrong-kernel models whose out AND out_aux planes are, bit for bit, what the launch wrote"""
    names = []
    for m in ref.MUTANTS:
        w = reference(case, mutant=m)
        if all(torch.equal(bits(got.view(o).cpu()), bits(w.view(o))) for o in ("out", "out_aux") if o in w.span):
            names.append(m)
    return names


def check(case, got, want):
    """every allocation of `got` (a Data after the launch, any device) holds the bits of `want`: the output planes the reference's,
    every operand, margin, padding column and unwritten plane the bits it started with.  The failure message names the mode, the
    first differing (frame, channel, pixel) with both values as hex, and the wrong-kernel model that reproduces the launch's bits."""
    bad = {n: m for n, m in differing(got, want).items() if m.any()}
    if not bad:
        return
    T, C, Npix, _ = case.shape
    lines = [f"{case.name}: mode {MODE_NAMES[case.mode]} ({case.entry} entry), {sum(int(m.sum()) for m in bad.values())} elements differ"]
    for name, m in sorted(bad.items()):
        at = int(torch.nonzero(m)[0])
        where = f"element {at - MARGIN} relative to the body (margin, padding or an operand)"
        for o in ("out", "out_aux"):
            a, start, n = want.span.get(o, (None, 0, 0))
            if a == name and start <= at < start + n:
                e = at - start
                where = f"{o} (frame {e // (C * Npix)}, channel {e // Npix % C}, pixel {e % Npix})"
        lines.append(f"  allocation {name}: {int(m.sum())} of {m.numel()}, first at {where}: got {_hex(got.allocs[name].cpu()[at])}, "
                     f"want {_hex(want.allocs[name][at])}")
    same = matching_mutants(case, got)
    lines.append("  the launch's output planes are those of the wrong-kernel model(s): " +
                 (", ".join(f"{m} ({ref.MUTANTS[m]})" for m in same) if same else "none of them"))
    raise AssertionError("\n".join(lines))


# ------------------------------------------------------------------------------------------------------------------------ the cases
def _tag(cfg, skip):
    return f"{'cfg' if cfg else 'nocfg'}-{'skip' if skip else 'eps'}"


def _shape_tag(s):
    return "T%dC%dN%dld%d" % s


def _cases():
    out = []
    for mode, mname in enumerate(MODE_NAMES):
        for shape in SHAPES:
            for cfg in (1, 0):
                for skip in (False, True):
                    z = 2 * cfg + skip
                    out.append(Case(f"{mname}-{_shape_tag(shape)}-{_tag(cfg, skip)}", f"grid-{mname}", mode, shape, cfg, skip, z=z))
                    if mode == HEUN1:
                        out.append(Case(f"euler-{_shape_tag(shape)}-{_tag(cfg, skip)}", "euler", HEUN1, shape, cfg, skip, z=z, entry="euler"))
    for cfg, skip in ((1, False), (0, True)):
        for n_hist in range(4):
            out.append(Case(f"LMS-hist{n_hist}-{_tag(cfg, skip)}", "lms-hist", LMS, cfg=cfg, skip=skip, n_hist=n_hist))
    for cfg in (1, 0):
        for skip in (False, True):
            out.append(Case(f"DPM2M-noaux-{_tag(cfg, skip)}", "dpm2m-noaux", DPM2M, cfg=cfg, skip=skip, with_aux=False))
        out.append(Case(f"LMS-negzero-{_tag(cfg, False)}", "lms-negzero", LMS, cfg=cfg, n_hist=0, special="negzero"))
    for mode, mname in enumerate(MODE_NAMES):
        for k, scale in enumerate((5.0, 1.0, 0.0, -1.5)):
            out.append(Case(f"{mname}-scale{scale:g}", "scale", mode, scale=scale, z=k))
        for skip in (False, True):
            out.append(Case(f"{mname}-unused-poisoned-{_tag(1, skip)}", "unused", mode, skip=skip, z=2 + skip, unused_poison=True))
    for skip in (False, True):
        out.append(Case(f"DPM2M-noaux-unused-poisoned-{_tag(1, skip)}", "unused", DPM2M, skip=skip, with_aux=False, unused_poison=True))
    for mode in (EULER_A, DPM2S_2):
        for k, s_noise in enumerate((0.9, 1.0, 0.0)):
            out.append(Case(f"{MODE_NAMES[mode]}-s_noise{s_noise:g}", "s_noise", mode, s_noise=s_noise, z=k))
    k = 0
    for mode, pairs in ((HEUN2, (("out", "x0"), ("out", "aux"))), (DPM2S_2, (("out", "x0"), ("out", "aux"))),
                        (DPM2M, (("out_aux", "aux"), ("out", "aux"))),
                        (LMS, tuple((o, f"hist{h}") for h in range(3) for o in ("out_aux", "out")))):
        for o, operand in pairs:
            out.append(Case(f"{MODE_NAMES[mode]}-alias-{o}={operand}", f"alias-{MODE_NAMES[mode]}", mode, z=k % 3, alias=((o, operand),)))
            k += 1
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
IDS = [c.name for c in CASES]
FAMILIES = sorted({c.family for c in CASES})
ALIASED = [c for c in CASES if c.alias]
EULER = [c for c in CASES if c.entry == "euler" and not c.unused_poison]
UNUSED = [c for c in CASES if c.unused_poison]


def base_of(case):
    """the case of an `unused` / euler case with None for every operand the mode does not read / through the struct entry: the same
    operands (data_key), so the same output bits"""
    return dataclasses.replace(case, unused_poison=False, entry="struct", name=case.name + "-base")
