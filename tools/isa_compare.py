"""Per-kernel comparison of two sets of device-only assembly listings of the kernel units; CPU only.
usage: python tools/isa_compare.py A B [--rename PATTERN REPLACEMENT]...

A / B: one side each, as a listing, several joined by commas (A1.s,A2.s) or a directory of *.s files. A listing is
`hipcc <build.py's kernel compile line> --cuda-device-only -S` of one unit of build.KERNEL_SOURCES; a side is one version
of all of them (or of some: e.g. the parent's single kernel file against the units it was split into). Prints the kernels
one side compiles twice (the same symbol in two of its listings: each kernel belongs to exactly one unit), the kernels only
one side has, the kernels whose instruction stream differs (with both lengths), and a one-line total. A
stream is the kernel's instructions and local labels: directives, comments and everything after ';' are dropped, and a
label's function number (.LBB<n>_<k>) is masked, since it only counts the kernels in front of this one. Streams are hashed
and compared whole; no instruction is looked for. Exit status 1 when anything differs or is compiled twice.
--rename: side A's symbols go through re.sub(PATTERN, REPLACEMENT) before the comparison, for a kernel whose mangled name
changed while its code should not have (a template parameter added to it); every symbol renamed is printed with its new name."""
import hashlib
import re
import sys
from pathlib import Path


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


def side(arg):
    """({kernel symbol: (instruction count, hash)} over the side's listings, how many symbols two of them hold)"""
    paths = sorted(map(str, Path(arg).glob("*.s"))) if Path(arg).is_dir() else arg.split(",")
    out, where, twice = {}, {}, 0
    for path in paths:
        for name, v in kernels(path).items():
            if name in out:
                twice += 1
                print(f"compiled twice: {name} in {where[name]} and {path}")
            out[name], where[name] = v, path
    return out, twice


def main(a_arg, b_arg, renames=()):
    (a, a_twice), (b, b_twice) = side(a_arg), side(b_arg)
    for pattern, repl in renames:
        for name in sorted(a):
            new = re.sub(pattern, repl, name)
            if new != name:
                print(f"renamed: {name}\n     ->  {new}")
                a[new] = a.pop(name)
    for name in sorted(set(a) - set(b)):
        print(f"only in {a_arg}: {name}")
    for name in sorted(set(b) - set(a)):
        print(f"only in {b_arg}: {name}")
    both = sorted(set(a) & set(b))
    differ = [k for k in both if a[k][1] != b[k][1]]
    for name in differ:
        print(f"differs: {name}  {a[name][0]} -> {b[name][0]} instructions")
    print(f"{len(a)} / {len(b)} kernels, {len(both)} in both, {len(both) - len(differ)} identical, {len(differ)} differ, "
          f"{len(set(a) ^ set(b))} in one only")
    print(f"{a_twice} / {b_twice} kernels compiled twice")
    return 1 if differ or set(a) ^ set(b) or a_twice or b_twice else 0


if __name__ == "__main__":
    rest = sys.argv[3:]
    if len(sys.argv) < 3 or len(rest) % 3 or any(rest[k] != "--rename" for k in range(0, len(rest), 3)):
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], [(rest[k + 1], rest[k + 2]) for k in range(0, len(rest), 3)]))
