"""Per-kernel resource table of the gfx950 code objects: VGPRs, SGPRs, spills, scratch, LDS, machine-code bytes.

    python tools/codeobj_stats.py [--digest] [source.hip ...]        (default: every source of panacea_amd/build.py)

Compiles each source device-only with the build's own flags (hipcc cross-compiles without a GPU), reads the
AMDGPU metadata notes and the symbol table with llvm-readelf.  The output committed under profiles/ is the evidence
for "no scratch, fits the instruction cache" claims.

--digest appends to each line twelve hex digits of the SHA-256 over the kernel's machine-code bytes in .text, and the source
the kernel was compiled in.  The hash is of the INSTRUCTIONS, not of where the linker put them: a kernel reaches its globals and
its callees pc-relative (s_getpc_b64, then s_add_u32 / s_addc_u32 with a 32-bit literal that is the distance from here to there),
and that distance moves when anything else in the translation unit does.  Those literals are zeroed before hashing
(placement_free), so one source line gives one digest in every translation unit that compiles it.  Tables written before this
masking (profiles/*_codeobj.txt up to gemm_dispatch_codeobj.txt) differ from today's in the kernels that hold such a sequence; run
the tool on both trees to compare.  Two trees whose tables agree line for line (after `sort`) in every column, digest included, ship the
same device code in the same translation units: the way a host-side or schedule-neutral refactor proves itself without a GPU.
Within a source the lines are ordered by code size, then name — not by the order in which the translation unit instantiates
its kernels.
"""
import hashlib
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from panacea_amd import build as B  # noqa: E402

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CXXFILT = "c++filt"


def device_elf(src: Path, tmp: Path) -> Path:
    co = tmp / (src.stem + ".co")
    subprocess.check_call([B._hipcc(), *B.FLAGS, "--offload-device-only", "-c", str(src), "-o", str(co)])
    data = co.read_bytes()
    elf = tmp / (src.stem + ".elf")
    elf.write_bytes(data[data.find(b"\x7fELF"):])
    return elf


def placement_free(code: bytes) -> bytes:
    """`code` with the literals of the s_add_u32 / s_addc_u32 that follow an s_getpc_b64 set to zero.  gfx9 encodings, one dword
    each: SOP1 s_getpc_b64 = 0xBE80_1C00 | sdst << 16; SOP2 = 0b10 op[29:23] sdst[22:16] ssrc1[15:8] ssrc0[7:0] with op 0 = s_add_u32,
    4 = s_addc_u32, and a source of 0xFF means that the next dword is the literal."""
    w = list(struct.unpack(f"<{len(code) // 4}I", code[:len(code) & ~3]))
    for i, d in enumerate(w):
        if d & 0xFF80FFFF != 0xBE801C00:
            continue
        j = i + 1
        while j + 1 < len(w) and w[j] & 0xFF800000 in (0x80000000, 0x82000000) and 0xFF in (w[j] & 0xFF, w[j] >> 8 & 0xFF):
            w[j + 1] = 0
            j += 2
    return struct.pack(f"<{len(w)}I", *w) + code[len(code) & ~3:]


def kernels(elf: Path):
    notes = subprocess.check_output([READELF, "--notes", str(elf)], text=True)
    syms = subprocess.check_output([READELF, "-sW", str(elf)], text=True)
    size, addr = {}, {}
    for ln in syms.splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]], addr[f[7]] = int(f[2]), int(f[1], 16)
    # .text: its address and file offset, for the bytes of a function
    text = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", subprocess.check_output([READELF, "-SW", str(elf)], text=True))
    text_addr, text_off = int(text.group(1), 16), int(text.group(2), 16)
    image = elf.read_bytes()
    out = []
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk)   # noqa: E731
        name = g("name").group(1)
        out.append(dict(name=name, vgpr=int(g("vgpr_count").group(1)), sgpr=int(g("sgpr_count").group(1)),
                        spill=int(g("vgpr_spill_count").group(1)), scratch=int(g("private_segment_fixed_size").group(1)),
                        lds=int(g("group_segment_fixed_size").group(1)), code=size.get(name, 0),
                        digest=hashlib.sha256(placement_free(image[text_off + addr.get(name, text_addr) - text_addr:][:size.get(name, 0)])).hexdigest()[:12]))
    return out


def short(name: str) -> str:
    d = subprocess.check_output([CXXFILT, name], text=True).strip()
    if d == name and "DF16_" in name:          # a c++filt that does not know _Float16's mangling: demangle it as `half`
        d = subprocess.check_output([CXXFILT, name.replace("DF16_", "Dh")], text=True).strip()
    d = re.sub(r"^void ", "", d).replace("pnc_gemm::", "").replace("(anonymous namespace)::", "")   # before the cut at the arguments
    return re.sub(r"\(.*$", "", d)


def main():
    args = [a for a in sys.argv[1:] if a != "--digest"]
    digest = len(args) != len(sys.argv[1:])
    srcs = [Path(a) for a in args] or [B.CSRC / s for s in B.SOURCES]
    worst = dict(spill=0, scratch=0, code=0)
    with tempfile.TemporaryDirectory() as td:
        print(f"{'kernel':86s} {'vgpr':>5s} {'sgpr':>5s} {'spill':>5s} {'scratch':>7s} {'code B':>8s}" + (f" {'sha256':>12s} source" if digest else ""))
        for s in srcs:
            for k in sorted(kernels(device_elf(s, Path(td))), key=lambda k: (-k["code"], k["name"])):
                print(f"{short(k['name'])[:86]:86s} {k['vgpr']:5d} {k['sgpr']:5d} {k['spill']:5d} {k['scratch']:7d} {k['code']:8d}" + (f" {k['digest']} {s.stem}" if digest else ""))
                for w in worst:
                    worst[w] = max(worst[w], k[w])
    print(f"max over all kernels: spill {worst['spill']}, scratch {worst['scratch']} B, code {worst['code']} B")


if __name__ == "__main__":
    main()
