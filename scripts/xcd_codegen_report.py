"""What the compiler made of the XCD-resident chunk kernel (ggad_amd/csrc/step_xcd.hip), per k_train_chunk_xcd instance:
registers, spills and private segment from the AMDGPU metadata, and from the assembly the vector-memory instructions inside the
step loop and how many of them are DIRECTLY followed by a full `s_waitcnt vmcnt(0)` (a dependent round trip on the step's
critical path unless the source means it).  Needs hipcc only, no GPU; compiles device-only into a temporary directory.

    python scripts/xcd_codegen_report.py [path/to/step_xcd.hip]      # e.g. a `git show REV:...` copy next to its headers
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggad_amd.build import CSRC, FLAGS, _hipcc  # noqa: E402

KERNEL = "k_train_chunk_xcd"
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
             ".group_segment_fixed_size")
VMEM = re.compile(r"^(global|flat|scratch|buffer)_(load|store|atomic)")      # vector memory (LDS and scalar loads are not counted)
FULL_WAIT = re.compile(r"^s_waitcnt\b.*vmcnt\(0\)")


def compile_asm(src: str, out_dir: str) -> str:
    asm = os.path.join(out_dir, "step_xcd.s")
    cmd = [_hipcc()] + FLAGS + ["-I", CSRC, "-x", "hip", "--cuda-device-only", "-S", src, "-o", asm]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return asm


def kernel_metadata(asm_text: str) -> dict:
    """{mangled name: {metadata key: int}} of every kernel of the code object (the .amdgpu_metadata YAML block)."""
    m = re.search(r"\.amdgpu_metadata\n(.*?)\n\s*\.end_amdgpu_metadata", asm_text, re.S)
    out = {}
    if not m:
        return out
    block = m.group(1)
    start = block.index("amdhsa.kernels:")
    end = block.find("\namdhsa.", start + 1)
    kernels = block[start:end if end > 0 else len(block)]
    for entry in re.split(r"\n  - ", kernels)[1:]:      # one list item per kernel; its scalar fields sit at four spaces
        fields = dict(re.findall(r"^\s{0,4}(\.[a-z_]+):\s+'?([^'\n]+)'?\s*$", "    " + entry, re.M))
        name = fields.get(".name")
        if name:
            out[name] = {k: int(fields[k]) for k in META_KEYS if k in fields and fields[k].lstrip("-").isdigit()}
    return out


def waves_per_simd(meta: dict) -> int:
    """gfx950: 512 unified registers per SIMD lane, allocated in blocks of 8; at most 8 waves."""
    regs = meta.get(".vgpr_count", 0)      # the unified total: it includes the accumulation registers
    blocks = max((regs + 7) // 8 * 8, 8)
    return min(8, 512 // blocks)


def function_body(asm_lines, name):
    try:
        i0 = asm_lines.index(name + ":") if name + ":" in asm_lines else next(i for i, l in enumerate(asm_lines) if l.startswith(name + ":"))
    except StopIteration:
        return []
    i1 = next(i for i in range(i0, len(asm_lines)) if asm_lines[i].startswith(".Lfunc_end"))
    return asm_lines[i0:i1]


def step_loop_stats(body):
    """Vector-memory instructions of the depth-1 loop that holds most of them (the step loop), and those directly followed by a
    full wait.  Blocks are attributed to their outermost loop by the comments llc writes behind block labels."""
    loops = {}
    cur = None
    insts = []      # (loop, mnemonic line)
    i = 0
    while i < len(body):
        line = body[i].strip()
        lab = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line)
        if lab:
            notes = [lab.group(2) or ""]
            j = i + 1
            while j < len(body) and body[j].strip().startswith(";"):
                notes.append(body[j].strip())
                j += 1
            text = " ".join(notes)
            top = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+) Depth=1\b", text)
            if top:
                cur = top.group(1)
            elif re.search(r"Loop Header: Depth=1\b", text):
                cur = lab.group(1)[2:]
            else:
                cur = None
            i = j
            continue
        if line and not line.startswith((";", ".")):
            insts.append((cur, line))
        i += 1
    for k, (loop, line) in enumerate(insts):
        if loop is None or not VMEM.match(line):
            continue
        st = loops.setdefault(loop, {"vmem": 0, "loads": 0, "full_wait_next": 0})
        st["vmem"] += 1
        st["loads"] += "_load" in line.split()[0]
        n = k + 1
        while n < len(insts) and insts[n][1].startswith("s_nop"):
            n += 1
        if n < len(insts) and insts[n][0] == loop and FULL_WAIT.match(insts[n][1]):
            st["full_wait_next"] += 1
    if not loops:
        return {"vmem": 0, "loads": 0, "full_wait_next": 0}
    return max(loops.values(), key=lambda s: s["vmem"])


def report(src: str):
    with tempfile.TemporaryDirectory() as tmp:
        text = open(compile_asm(src, tmp)).read()
    lines = text.split("\n")
    rows = []
    for name, meta in sorted(kernel_metadata(text).items()):
        if KERNEL not in name:
            continue
        inst = re.search(r"ILi(\d+)ELi(\d+)E", name)
        st = step_loop_stats(function_body(lines, name))
        rows.append({"instance": f"<{inst.group(1)},{inst.group(2)}>" if inst else name, "name": name, "meta": meta, "waves_per_simd": waves_per_simd(meta),
                     "loop": st})
    return rows


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(CSRC, "step_xcd.hip")
    print(f"{KERNEL}: hipcc {' '.join(FLAGS)} --cuda-device-only -S")
    print(f"{'instance':10s} {'VGPRs':>6s} {'VGPR spills':>12s} {'SGPR spills':>12s} {'private bytes':>14s} {'waves/SIMD':>11s} "
          f"{'loop vmem':>10s} {'loop loads':>11s} {'+ full wait':>12s}")
    for r in report(src):
        m, st = r["meta"], r["loop"]
        print(f"{r['instance']:10s} {m.get('.vgpr_count', -1):6d} {m.get('.vgpr_spill_count', -1):12d} {m.get('.sgpr_spill_count', -1):12d} "
              f"{m.get('.private_segment_fixed_size', -1):14d} {r['waves_per_simd']:11d} {st['vmem']:10d} {st['loads']:11d} {st['full_wait_next']:12d}")
    print("loop vmem / loads: global, flat, scratch and buffer instructions inside the step loop; + full wait: those whose next instruction is "
          "s_waitcnt vmcnt(0)")


if __name__ == "__main__":
    main()
