"""Build tools/bz_check.cpp with AddressSanitizer and UBSan and run it over the
bzip2 decoder's case list (tests/bz_cases.py): the valid files, the corrupt
ones, every single-bit flip and truncation of a small file, and the chain
logic with a false and with a missing candidate.  A host program on the CPU:
it needs no device and is not meant for a GPU machine.

  python tools/bz_check.py [--keep DIR]
"""
import bz2
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_cases(d):
    from tests import bz_cases
    lines = []
    for name in bz_cases.VALID_NAMES:
        plain, z = bz_cases.valid_cases()[name]
        open(os.path.join(d, name + ".bz2"), "wb").write(z)
        open(os.path.join(d, name + ".out"), "wb").write(plain)
        lines.append(f"valid {name} 0")
    for name in bz_cases.CORRUPT_NAMES:
        z, reason = bz_cases.corrupt_cases()[name]
        open(os.path.join(d, name + ".bz2"), "wb").write(z)
        lines.append(f"corrupt {name} {-1 if reason is None else reason}")
    # small enough for a few thousand mutations: two streams, runs, a count byte
    small = bz_cases.wiggle_text(700, seed=3) + b"a" * 300 + bytes(range(40)) + b"\n"
    open(os.path.join(d, "small.bz2"), "wb").write(bz2.compress(small[:500]) + bz2.compress(small[500:], 1))
    lines.append("fuzz small 0")
    plain, z = bz_cases.valid_cases()["wiggle_level1"]
    open(os.path.join(d, "chain.bz2"), "wb").write(z)
    open(os.path.join(d, "chain.out"), "wb").write(plain)
    lines.append("chain chain 0")
    open(os.path.join(d, "manifest.txt"), "w").write("\n".join(lines) + "\n")


def main():
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    with tempfile.TemporaryDirectory() as tmp:
        d = keep or tmp
        os.makedirs(d, exist_ok=True)
        write_cases(d)
        exe = os.path.join(d, "bz_check")
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
               "-o", exe, os.path.join(ROOT, "tools", "bz_check.cpp")]
        print("+", " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        return subprocess.run([exe, d]).returncode


if __name__ == "__main__":
    sys.exit(main())
