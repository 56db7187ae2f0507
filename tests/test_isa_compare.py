"""tools/isa_compare.py on made-up listings (CPU only): sides of several listings, a kernel held by two listings of a side."""
import subprocess
import sys
from pathlib import Path

TOOL = Path(__file__).resolve().parent.parent / "tools" / "isa_compare.py"


def listing(*kernels):
    """A device listing with the kernels (name, instructions); local labels carry the kernel's number in the file."""
    out = []
    for n, (name, body) in enumerate(kernels):
        out += [f"\t.globl\t{name}", f"{name}:", f".LBB{n}_0:", *(f"\t{i} ; comment" for i in body), f"\ts_cbranch_scc1 .LBB{n}_0", "\ts_endpgm",
                f".Lfunc_end{n}:", f"\t.amdhsa_kernel {name}", "\t.end_amdhsa_kernel"]
    return "\n".join(out) + "\n"


def run(*args):
    r = subprocess.run([sys.executable, str(TOOL), *map(str, args)], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_one_file_against_the_units_it_was_cut_into(tmp_path):
    ka, kb, kc = ("k_a", ["v_add_f64 v[0:1], v[0:1], v[2:3]"]), ("k_b", ["s_nop 0", "s_nop 1"]), ("k_c", ["v_mov_b32 v0, 0"])
    (tmp_path / "whole.s").write_text(listing(ka, kb, kc))
    units = tmp_path / "units"
    units.mkdir()
    (units / "u1.s").write_text(listing(kc, ka))  # another order: the labels' function numbers differ
    (units / "u2.s").write_text(listing(kb))
    want = "3 / 3 kernels, 3 in both, 3 identical, 0 differ, 0 in one only\n0 / 0 kernels compiled twice\n"
    assert run(tmp_path / "whole.s", units) == (0, want)
    assert run(tmp_path / "whole.s", f"{units / 'u1.s'},{units / 'u2.s'}") == (0, want)


def test_a_kernel_in_two_listings_of_a_side_a_changed_and_a_missing_one(tmp_path):
    ka, kb = ("k_a", ["s_nop 0"]), ("k_b", ["s_nop 0", "s_nop 1"])
    (tmp_path / "whole.s").write_text(listing(ka, kb))
    (tmp_path / "u1.s").write_text(listing(ka))
    (tmp_path / "u2.s").write_text(listing(kb, ka))
    code, out = run(tmp_path / "whole.s", f"{tmp_path / 'u1.s'},{tmp_path / 'u2.s'}")
    assert code == 1 and f"compiled twice: k_a in {tmp_path / 'u1.s'} and {tmp_path / 'u2.s'}" in out
    assert out.endswith("2 / 2 kernels, 2 in both, 2 identical, 0 differ, 0 in one only\n0 / 1 kernels compiled twice\n")
    (tmp_path / "u3.s").write_text(listing(("k_b", ["s_nop 0", "s_nop 1", "s_nop 2"])))
    code, out = run(tmp_path / "whole.s", tmp_path / "u3.s")
    assert code == 1 and "differs: k_b  4 -> 5 instructions" in out and f"only in {tmp_path / 'whole.s'}: k_a" in out
    assert out.endswith("2 / 1 kernels, 1 in both, 0 identical, 1 differ, 1 in one only\n0 / 0 kernels compiled twice\n")
