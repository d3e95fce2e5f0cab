"""Static instruction mix of gfx950 kernels, per kernel: total instructions,
VALU instructions (v_*), v_mad_u64_u32, v_lshl_add_u64, s_nop, scratch
accesses (scratch_load_* / scratch_store_*), and the .vgpr_count,
.vgpr_spill_count and .private_segment_fixed_size notes.

Usage:
  python tools/isa_mix.py FILE.s                      assembly of `hipcc -S --cuda-device-only`
  python tools/isa_mix.py FILE.hip -- FLAGS...        compiles FILE.hip to assembly with FLAGS first
  python tools/isa_mix.py --unit k_decode [MAKEVARS]  FILE = cess_amd/csrc/k_decode.hip, FLAGS from
                                                      `make -s print-kflags-k_decode MAKEVARS`
  python tools/isa_mix.py FILE.o | FILE.so            the gfx950 code objects bundled in an object
                                                      file or library, disassembled
Options: --filter SUBSTR (kernel names), --label TEXT (first column).
Only kernels (symbols with an AMDGPU metadata entry) are listed; a device
function the compiler did not inline is counted with no kernel."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cess_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BIN = "/opt/rocm/lib/llvm/bin"
NOTES = (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")
COLS = ("total", "valu", "v_mad_u64_u32", "v_lshl_add_u64", "s_nop", "scratch")

LABEL_S = re.compile(r"^([A-Za-z_$][\w$.]*):")                  # assembly: `name:`
LABEL_D = re.compile(r"^[0-9a-f]+ <([A-Za-z_$][\w$.]*)>:")      # disassembly: `0000 <name>:`
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def count(lines, disasm):
    """{symbol: {column: count}} for every function label of an assembly or disassembly text."""
    out, cur = {}, None
    label = LABEL_D if disasm else LABEL_S
    for line in lines:
        m = label.match(line)
        if m:
            name = m.group(1)
            if not name.startswith(".L") and not name.startswith("L"):
                cur = out.setdefault(name, dict.fromkeys(COLS, 0))
            continue
        if not disasm and re.match(r"^\.Lfunc_end", line):
            cur = None
            continue
        m = INSTR.match(line)
        if not m or cur is None:
            continue
        op = m.group(1)
        if op == "s_code_end":
            continue
        if op == "s_nop" and disasm:      # alignment padding behind a function's last instruction is not counted
            cur["_pad"] = cur.get("_pad", 0) + 1
            continue
        if cur.get("_pad"):
            cur["total"] += cur["_pad"]
            cur["s_nop"] += cur.pop("_pad")
        cur["total"] += 1
        if op.startswith("v_"):
            cur["valu"] += 1
        if op in ("v_mad_u64_u32", "v_lshl_add_u64", "s_nop"):
            cur[op] += 1
        if op.startswith("scratch_load") or op.startswith("scratch_store"):
            cur["scratch"] += 1
    return out


def notes_of(text):
    """{kernel: {note: value}} from AMDGPU metadata (assembly's .amdgpu_metadata or llvm-readelf --notes)."""
    out, vals = {}, {}
    for line in text.splitlines():
        s = line.strip().lstrip("- ").strip()
        k, _, v = s.partition(":")
        if k in NOTES or k == ".symbol":
            vals[k] = v.strip().strip("'\"")
        if k == ".wavefront_size":        # last key of one kernel's entry; .symbol is `<kernel>.kd`
            out[vals.get(".symbol", "")[:-3]] = {n: vals.get(n, "-") for n in NOTES}
            vals = {}
    return out


def short_name(sym):
    """The (possibly nested) function name of an Itanium-mangled symbol, without its parameter types."""
    m = re.match(r"_ZN?", sym)
    if not m:
        return sym
    parts, p = [], m.end()
    while True:
        d = re.match(r"\d+", sym[p:])
        if not d:
            break
        p += d.end()
        parts.append(sym[p:p + int(d.group())])
        p += int(d.group())
        if not m.group().endswith("N"):
            break
    return "::".join(parts) or sym


def demangle(names):
    return {n: short_name(n) for n in names}


def mix_of_asm(path):
    text = open(path).read()
    return count(text.splitlines(), False), notes_of(text)


def mix_of_binary(path):
    counts, notes = {}, {}
    with tempfile.TemporaryDirectory() as t:
        b = os.path.join(t, "bundle")
        shutil.copy(path, b)
        subprocess.check_call([os.path.join(BIN, "llvm-objdump"), "--offloading", b], cwd=t, stdout=subprocess.DEVNULL)
        for o in sorted(glob.glob(b + ".*gfx950*")):
            d = subprocess.run([os.path.join(BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", o], capture_output=True,
                               text=True, check=True).stdout
            counts.update(count(d.splitlines(), True))
            n = subprocess.run([os.path.join(BIN, "llvm-readelf"), "--notes", o], capture_output=True, text=True,
                               check=True).stdout
            notes.update(notes_of(n))
    return counts, notes


def compile_to_asm(src, flags, out):
    subprocess.check_call([HIPCC] + flags + ["-S", "--cuda-device-only", "-I", CSRC, src, "-o", out])


def unit_flags(unit, makevars):
    r = subprocess.run(["make", "-s", "-C", CSRC, "print-kflags-" + unit] + makevars, capture_output=True, text=True,
                       check=True)
    return r.stdout.split()


def rows(counts, notes, flt=""):
    names = demangle([k for k in counts if k in notes])
    shorts = list(names.values())
    names = {k: v if shorts.count(v) == 1 else f"{v}[{k}]" for k, v in names.items()}   # template instances
    for k in sorted(names, key=lambda k: names[k]):
        if flt in names[k]:
            yield names[k], counts[k], notes[k]


def main():
    argv = sys.argv[1:]
    flags = []
    if "--" in argv:
        i = argv.index("--")
        argv, flags = argv[:i], argv[i + 1:]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", nargs="?")
    ap.add_argument("makevars", nargs="*", help="with --unit: VAR=value arguments passed to make")
    ap.add_argument("--unit")
    ap.add_argument("--filter", default="")
    ap.add_argument("--label", default="")
    a = ap.parse_args(argv)
    if a.unit:
        src = os.path.join(CSRC, a.unit + ".hip")
        flags = unit_flags(a.unit, ([a.file] if a.file else []) + a.makevars)
    elif a.file:
        src = a.file
    else:
        ap.error("FILE or --unit")
    if src.endswith(".s"):
        counts, notes = mix_of_asm(src)
    elif src.endswith((".o", ".so")):
        counts, notes = mix_of_binary(src)
    else:
        with tempfile.TemporaryDirectory() as t:
            s = os.path.join(t, "unit.s")
            compile_to_asm(src, flags, s)
            counts, notes = mix_of_asm(s)
    lab = (a.label + " ") if a.label else ""
    print(f"# {lab}kernel total valu v_mad_u64_u32 v_lshl_add_u64 s_nop scratch_accesses vgpr_count vgpr_spill_count "
          f"private_segment_fixed_size")
    for name, c, n in rows(counts, notes, a.filter):
        print(lab + name + " " + " ".join(str(c[k]) for k in COLS) + " " + " ".join(n[k] for k in NOTES))


if __name__ == "__main__":
    main()
