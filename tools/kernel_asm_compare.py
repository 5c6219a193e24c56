"""Whether two builds of one HIP source hold the same kernels, instruction for instruction.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -S --cuda-device-only SOURCE.hip -o new.s      (the same at the other commit: old.s)
    python tools/kernel_asm_compare.py old.s new.s

Kernels are matched by their name and their boolean template arguments; a kernel with fewer arguments in one file is matched as if the missing ones
were false (a template argument added with the default false).  Compared are the instructions and their operands; comments, directives and the numbering
of the basic-block labels (which counts the functions in front) are not.  One line per kernel of new.s; exit status 1 if a matched kernel differs."""
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if t and (not t.startswith(".") or t.startswith(".LBB")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def key(symbol, n_flags):
    m = re.search(r"\d+([a-z0-9_]+_kernel)(?:I((?:Lb[01]E)+)E)?", symbol)
    flags = re.findall(r"Lb([01])E", m.group(2) or "") if m else []
    return (m.group(1) if m else symbol, tuple(flags + ["0"] * (n_flags - len(flags))) if flags else ())


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    n_flags = max([len(key(k, 0)[1]) for k in list(old) + list(new)] + [0])
    old = {key(k, n_flags): v for k, v in old.items()}
    differs = False
    for sym, text in new.items():
        k = key(sym, n_flags)
        name = k[0] + ("<" + ", ".join(k[1]) + ">" if k[1] else "")
        if k not in old:
            print(f"{name:44s} {len(text):6d} instructions and labels, new")
        elif old[k] == text:
            print(f"{name:44s} {len(text):6d} instructions and labels, identical")
        else:
            differs = True
            print(f"{name:44s} {len(text):6d} instructions and labels, DIFFERENT ({len(old[k])} before)")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
