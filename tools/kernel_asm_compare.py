"""Whether two builds of one HIP source hold the same kernels, instruction for instruction.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -S --cuda-device-only SOURCE.hip -o new.s      (the same at the other commit: old.s)
    python tools/kernel_asm_compare.py [--diff] old.s new.s

Kernels are matched by their full mangled symbol where both files have it (every instance of a template is a kernel of its own).  A symbol that only one file
has is matched by its name and its boolean template arguments, a kernel with fewer arguments in one file as if the missing ones were false (a template argument
added with the default false; a kernel that was no template at all as the instance with every argument false).  Compared are the instructions and their operands -- comments, directives and the numbering of the basic-block labels (which
counts the functions in front) are not -- and the kernel descriptor's register, LDS and scratch sizes.  One line per kernel of new.s, the sizes where they
differ, with --diff the differing lines; exit status 1 if a matched kernel differs."""
import difflib
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """symbol -> (instructions and labels, {resource: value})"""
    text, res, cur, desc = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = text.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            desc = res.setdefault(m.group(1), {})
            continue
        if desc is not None:
            m = re.match(r"^\s*\.amdhsa_(\w+)\s+(\S+)", line)
            if m and m.group(1) in RESOURCES:
                desc[m.group(1)] = m.group(2)
            elif line.strip() == ".end_amdhsa_kernel":
                desc = None
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if t and (not t.startswith(".") or t.startswith(".LBB")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return {k: (v, res.get(k, {})) for k, v in text.items()}


def key(symbol, n_flags):
    m = re.search(r"\d+([a-z0-9_]+kernel)(?:I((?:Lb[01]E)+)E)?", symbol)
    flags = re.findall(r"Lb([01])E", m.group(2) or "") if m else []
    return (m.group(1) if m else symbol, tuple(flags + ["0"] * (n_flags - len(flags))))      # (a kernel that was no template before: all false)


def shown(symbol):
    """_Z17conv_chain_kernelILi3EEv13ConvChainArgs -> conv_chain_kernel<3>"""
    m = re.match(r"_Z(\d+)", symbol)
    if not m:
        return symbol
    end = m.end() + int(m.group(1))
    rest = symbol[end:]
    t = re.match(r"I((?:L[a-z]n?\d+E)+)E", rest)
    if t:                                                           # integer and bool literals (n: negative)
        return symbol[m.end():end] + "<" + ", ".join(v.replace("n", "-") for v in re.findall(r"L[a-z](n?\d+)E", t.group(1))) + ">"
    return symbol[m.end():end] + (f"<{symbol}>" if rest.startswith("I") else "")      # other template arguments: the whole symbol tells the instances apart


def main():
    args = [a for a in sys.argv[1:] if a != "--diff"]
    old, new = kernels(args[0]), kernels(args[1])
    lone = [k for k in old if k not in new] + [k for k in new if k not in old]      # matched by name and flags
    n_flags = max([len(key(k, 0)[1]) for k in lone] + [0])
    old_lone = {key(k, n_flags): v for k, v in old.items() if k not in new}
    differs = False
    for sym, (text, res) in new.items():
        before = old.get(sym) or old_lone.get(key(sym, n_flags))
        name = shown(sym)
        if before is None:
            print(f"{name:44s} {len(text):6d} instructions and labels, new")
            continue
        same = before[0] == text
        print(f"{name:44s} {len(text):6d} instructions and labels, " + ("identical" if same else f"DIFFERENT ({len(before[0])} before)"))
        for r in RESOURCES:
            if before[1].get(r) != res.get(r):
                same = False
                print(f"    {r}: {before[1].get(r)} -> {res.get(r)}")
        if before[0] != text and "--diff" in sys.argv:
            for d in difflib.unified_diff(before[0], text, "old", "new", n=0, lineterm=""):
                print("    " + d)
        differs |= not same
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
