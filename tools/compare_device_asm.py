"""Kernel-by-kernel comparison of the device assembly of two builds: a refactor's proof that it left the code alone.

  make -C pigeon.jl_amd/csrc pg_api.s pg_api_f32.s          (at both commits, one of them in a scratch copy)
  python tools/compare_device_asm.py OLD/pg_api.s NEW/pg_api.s [--rename OLD=NEW ...] [--allow-different NAME ...] [--diff N]

Kernels are matched by demangled name without return type and parameter list (`pg::k_advance`, `pg::k_node_finish<true>`).  `--rename OLD=NEW` replaces the
prefix OLD of a name of the first file by NEW before matching (a kernel that became a template instantiation: 'pg::k_advance_dist=pg::k_advance_lib<double const* restrict>'; float in the fp32 pair).
Per kernel: identical / different / only in one file, and next_free_vgpr / next_free_sgpr / private segment size of both sides.
IDENTICAL: the lines from the kernel's label to its .Lfunc_end -- instructions and the .amdhsa_* block, .amdhsa_kernarg_size included -- are equal after removing
comments, renumbering the labels of the function (.LBB<n>_<k> -> .LBB_<k>) and replacing the kernel's own symbol.  Section switches (`.section`, `.text`) are left out:
which section holds code and descriptor is linkage (a template instantiation lives in a COMDAT group named after it), not code.  This diffs text; it looks for no instruction.
Exit status 1 when a kernel outside --allow-different differs or exists in one file only."""
import argparse
import difflib
import re
import shutil
import subprocess
import sys


def kernels(path):
    """{symbol: normalised lines from its label to .Lfunc_end} of the kernels (symbols with an .amdhsa_kernel block) of one .s file"""
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), []
        elif cur and line.startswith(".Lfunc_end"):
            if any(l.startswith(".amdhsa_kernel ") for l in body):
                out[cur] = body
            cur = None
        elif cur:
            t = line.split(";")[0].strip().replace(cur, "@KERNEL")
            if t and not t.startswith(".section") and t != ".text":
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        sys.exit("compare_device_asm: needs llvm-cxxfilt or c++filt")
    names = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(symbols, map(short_name, names)))


def short_name(demangled):
    """'void pg::k<true>(pg::DevCfg, int)' -> 'pg::k<true>': cut at the parameter list (the first '(' outside <>), drop the return type"""
    depth = 0
    for i, c in enumerate(demangled):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            demangled = demangled[:i]
            break
    depth = 0
    for i in range(len(demangled) - 1, -1, -1):
        c = demangled[i]
        depth += (c == ">") - (c == "<")
        if c == " " and depth == 0:
            return demangled[i + 1:]
    return demangled


def figures(body):
    get = lambda key: next((l.split()[1] for l in body if l.startswith(key + " ")), "?")
    return "vgpr %s sgpr %s scratch %s" % (get(".amdhsa_next_free_vgpr"), get(".amdhsa_next_free_sgpr"), get(".amdhsa_private_segment_fixed_size"))


def load(path, renames=()):
    ks = kernels(path)
    by_name = {}
    for sym, name in demangle(list(ks)).items():
        for old, new in renames:
            if name.startswith(old):
                name = new + name[len(old):]
                break
        if name in by_name:
            sys.exit(f"compare_device_asm: two kernels of {path} are both called {name}")
        by_name[name] = ks[sym]
    return by_name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--rename", nargs="+", action="extend", default=[], metavar="OLD=NEW")
    ap.add_argument("--allow-different", nargs="*", default=[], metavar="NAME")
    ap.add_argument("--diff", type=int, default=0, metavar="N", help="print the first N lines of the diff of a kernel that differs")
    a = ap.parse_args()
    old, new = load(a.old, [r.split("=", 1) for r in a.rename]), load(a.new)
    count = {"identical": 0, "different": 0, "only in old": 0, "only in new": 0}
    failed = False
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        verdict = "only in new" if o is None else "only in old" if n is None else "identical" if o == n else "different"
        count[verdict] += 1
        failed |= verdict != "identical" and name not in a.allow_different
        print(f"{verdict:12s} {name}: " + " | ".join(figures(b) for b in (o, n) if b is not None))
        if verdict == "different":
            for line in list(difflib.unified_diff(o, n, "old", "new", lineterm="", n=0))[:a.diff]:
                print("    " + line)
    print(f"{a.old} -> {a.new}: " + ", ".join(f"{v} {k}" for k, v in count.items()))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
