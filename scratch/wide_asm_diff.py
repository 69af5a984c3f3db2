"""Compare the device assembly of dc_mfma_wide.hip before and after a change, kernel by kernel, and print the resources
of the instances from the code object's metadata.

    hipcc <the library's flags> --cuda-device-only -S -o before.s dc_mfma_wide.hip     (in the parent's tree)
    hipcc <the library's flags> --cuda-device-only -S -o after.s  dc_mfma_wide.hip
    python scratch/wide_asm_diff.py before.s after.s

A kernel is named by the template arguments of its symbol (wide_sweep_kernel<MODE, NR, SM, PR>) or, for the other kernels
and the noinline functions, by its function name: the rest of the mangled name spells the parameter type, which changes
whenever WideKernelArgs gains a parameter without the instance changing.  The body compared is every instruction line
between the label and .Lfunc_end, with symbol names replaced by that short name and comments dropped."""
import re
import sys


def short(sym):
    m = re.match(r"_ZN2dc12_GLOBAL__N_1(\d+)", sym)
    if not m:
        return sym
    n = int(m.group(1))
    name = sym[m.end():m.end() + n]
    rest = sym[m.end() + n:]
    t = re.match(r"I((?:L[A-Za-z0-9_]*?E)+)E", rest)
    return name + ("<" + t.group(1) + ">" if t else "")


def functions(path):
    out, cur, body = {}, None, []
    syms = set()
    lines = open(path).read().split("\n")
    for ln in lines:
        m = re.match(r"(_Z\w+):\s", ln + " ")
        if m and cur is None:
            cur, body = m.group(1), []
            syms.add(cur)
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[cur] = body
                cur = None
                continue
            code = ln.split(";")[0].rstrip()
            if code.strip() and not code.lstrip().startswith("."):
                body.append(code)
            elif re.match(r"\.LBB\d+_\d+:", code.strip()):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", code.strip()))
    named = {}
    for sym, body in out.items():
        text = "\n".join(body)
        for s in sorted(syms, key=len, reverse=True):
            text = text.replace(s, short(s))
        text = re.sub(r"\.LBB\d+_", ".LBB_", text)
        assert short(sym) not in named, short(sym)
        named[short(sym)] = text
    return named


def metadata(path):
    """kernel -> (vgpr, agpr, spill, private bytes, LDS bytes) from the amdhsa.kernels notes"""
    res = {}
    text = open(path).read()
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        blk = ".agpr_count:" + blk
        def f(k):
            m = re.search(r"\." + k + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        res[short(f("name"))] = tuple(f(k) for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                                      "group_segment_fixed_size"))
    return res


def main():
    before, after = functions(sys.argv[1]), functions(sys.argv[2])
    same = [k for k in before if k in after and before[k] == after[k]]
    changed = [k for k in before if k in after and before[k] != after[k]]
    print("identical, instruction for instruction: %d of %d" % (len(same), len(before)))
    for k in sorted(same):
        print("  =", k, "(%d lines)" % (before[k].count("\n") + 1))
    for k in sorted(changed):
        print("  CHANGED", k, "(%d -> %d lines)" % (before[k].count("\n") + 1, after[k].count("\n") + 1))
    for k in sorted(set(before) - set(after)):
        print("  GONE", k)
    md = metadata(sys.argv[2])
    print("new (vgpr, agpr, spill, private, LDS):")
    for k in sorted(set(after) - set(before)):
        print("  +", k, md.get(k, ""))
    return 1 if changed or set(before) - set(after) else 0


if __name__ == "__main__":
    sys.exit(main())
