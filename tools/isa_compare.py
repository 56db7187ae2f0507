"""Per-kernel comparison of two device-only assembly listings of the kernel file; CPU only.
usage: python tools/isa_compare.py A.s B.s

A.s / B.s: `hipcc <build.py's kernel compile line> --cuda-device-only -S` of two versions of rtc_kernels.hip. Prints the
kernels only one of them has, the kernels whose instruction stream differs (with both lengths), and a one-line total. A
stream is the kernel's instructions and local labels: directives, comments and everything after ';' are dropped, and a
label's function number (.LBB<n>_<k>) is masked, since it only counts the kernels in front of this one. Streams are hashed
and compared whole; no instruction is looked for. Exit status 1 when anything differs."""
import hashlib
import re
import sys


def kernels(path):
    """{kernel symbol: (instruction count, hash of the stream)}"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, stream = {}, None, []
    for line in text.split("\n"):
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur, stream = line[:-1], []
            continue
        if line.startswith(".Lfunc_end"):
            n = sum(1 for s in stream if not s.endswith(":"))
            out[cur] = (n, hashlib.sha256("\n".join(stream).encode()).hexdigest())
            cur = None
        elif line.endswith(":") or not line.startswith("."):  # a local label or an instruction; directives go
            stream.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    for name in sorted(set(a) - set(b)):
        print(f"only in {a_path}: {name}")
    for name in sorted(set(b) - set(a)):
        print(f"only in {b_path}: {name}")
    both = sorted(set(a) & set(b))
    differ = [k for k in both if a[k][1] != b[k][1]]
    for name in differ:
        print(f"differs: {name}  {a[name][0]} -> {b[name][0]} instructions")
    print(f"{len(a)} / {len(b)} kernels, {len(both)} in both, {len(both) - len(differ)} identical, {len(differ)} differ, "
          f"{len(set(a) ^ set(b))} in one only")
    return 1 if differ or set(a) ^ set(b) else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
