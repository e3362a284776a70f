#!/usr/bin/env python3
"""Compare kernels' machine code between two device code objects.

    hipcc --offload-arch=gfx950 <build.py's flags> --offload-device-only -c UNIT.hip -o a.co   (each tree)
    tools/kernel_disasm_diff.py a.co b.co mc_frames_kernel

Disassembles both with llvm-objdump, takes every function whose (mangled) name contains
the pattern, strips what a change elsewhere in the unit moves -- instruction addresses,
encodings, branch-target labels' addresses -- and prints a unified diff of the instruction
text per function, then one summary line per function: identical, or the number of
differing lines.  Exit status 1 if any function differs or is missing on one side."""
import difflib
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
BUNDLER = "/opt/rocm/lib/llvm/bin/clang-offload-bundler"


def code_object(path):
    """The gfx code object of `path`: the file itself, or the device part of an offload bundle (what
    `--offload-device-only -c` writes), unbundled into a temporary file."""
    with open(path, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return path
    listing = subprocess.run([BUNDLER, "--list", "--type=o", f"--input={path}"], check=True, capture_output=True, text=True)
    target = next(t for t in listing.stdout.split() if t.startswith("hip"))
    out = tempfile.NamedTemporaryFile(suffix=".co", delete=False).name
    subprocess.run([BUNDLER, "--unbundle", "--type=o", f"--targets={target}", f"--input={path}", f"--output={out}"], check=True)
    return out


def functions(path, pattern):
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", code_object(path)], check=True, capture_output=True,
                          text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1) if pattern in m.group(1) else None
            if name:
                out[name] = []
            continue
        if name is None or not line.strip():
            continue
        ins = re.sub(r"//.*$", "", line).strip()            # the address / encoding comment
        ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)             # a leading address
        ins = re.sub(r"<([^>+]+)\+0x[0-9a-f]+>", r"<\1+OFF>", ins)  # branch targets: symbol + offset
        ins = re.sub(r"\b0x[0-9a-f]+ <", "ADDR <", ins)
        out[name].append(ins)
    return out


def main():
    a, b, pattern = sys.argv[1:4]
    fa, fb = functions(a, pattern), functions(b, pattern)
    bad = 0
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            print(f"{name}: only in {'the first' if name in fa else 'the second'}")
            bad += 1
            continue
        d = list(difflib.unified_diff(fa[name], fb[name], "a", "b", lineterm="", n=2))
        n = sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))
        if n:
            print("\n".join(d))
            bad += 1
        print(f"{name}: {len(fa[name])} / {len(fb[name])} instructions, " + ("identical" if not n else f"{n} differing lines"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
