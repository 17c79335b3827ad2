"""Offline table of the register epilogue's recipes: reads the gfx950 assembly of conv_fprop kernels and prints, per kernel, its
size, its main-loop block and -- for every epilogue recipe the kernel carries -- the instructions and conditional branches of that recipe's code.  No GPU needed.

    hipcc <the flags of synthanatomy_amd/build.py> -DSA_EPI_MARKERS --cuda-device-only -S kernels.hip -o kernels.s
    python tools/epilogue_paths.py kernels.s [more.s ...]

-DSA_EPI_MARKERS (csrc/conv_fprop_common.h) puts an assembler comment, no instruction, in front of and behind every recipe; a recipe's code is what lies
between its two comments; a recipe whose comments enclose another recipe's is starred (the two are laid out interleaved and the count is an upper bound).
Without the markers only the kernel totals are printed (the parent commit).
"""
import re
import sys

FUNC = re.compile(r"^(_ZN2sa\w+):")
MARK = re.compile(r"^\s*; SA_RECIPE_(BEGIN|END) (\d)")


def kernels(path):
    """{kernel symbol: [instruction or marker, ...]} -- labels, directives and comments dropped"""
    out, cur = {}, None
    for line in open(path):
        m = MARK.match(line)
        s = line.split(";")[0].strip()
        f = FUNC.match(s)
        if f:
            cur = out.setdefault(f.group(1), [])
        elif cur is None:
            continue
        elif m:
            cur.append((m.group(1), int(m.group(2))))
        elif s.startswith((".Lfunc_end", ".section")):
            cur = None
        elif s and not s.startswith(".") and not s.endswith(":"):
            cur.append(s)
    return out


def main():
    print(f"{'kernel':70s} {'instr':>6s} {'cbranch':>7s} {'loop MFMA/VALU/LDS':>19s}  recipe: instructions/conditional branches")
    for path in sys.argv[1:]:
        for name, body in kernels(path).items():
            ins = [s for s in body if isinstance(s, str)]
            # the main loop: the run of instructions between two branches with 32 MFMAs (one slab step; the fused block's unrolled second product has 64)
            runs, cur = [], []
            for s in ins:
                cur.append(s)
                if s.startswith(("s_branch", "s_cbranch", "s_endpgm")):
                    runs.append(cur)
                    cur = []
            loop = max(runs, key=lambda r: (sum(s.startswith("v_mfma") for s in r) == 32, sum(s.startswith("v_mfma") for s in r)))
            lp = (sum(s.startswith("v_mfma") for s in loop), sum(s.startswith("v_") and not s.startswith("v_mfma") for s in loop),
                  sum(s.startswith("ds_read") for s in loop))
            # (the compiler may lay two recipes' blocks out interleaved: such a recipe counts everything between its comments, an upper bound, and is starred)
            cols, live = [], {}
            for s in body:
                if isinstance(s, tuple):
                    if s[0] == "BEGIN":
                        assert s[1] not in live and s[1] not in {r for r, _, _, _ in cols}, "a recipe's code appears twice"
                        live[s[1]] = [0, 0, bool(live)]
                        for v in list(live.values())[:-1]:
                            v[2] = True
                    else:
                        n, c, mixed = live.pop(s[1])
                        cols.append((s[1], n, c, mixed))
                else:
                    for v in live.values():
                        v[0] += 1
                        v[1] += s.startswith("s_cbranch")
            assert not live, "a recipe's closing comment is missing"
            txt = "  ".join(f"{r}: {n}/{c}{'*' if mixed else ''}" for r, n, c, mixed in sorted(cols))
            print(f"{name[:70]:70s} {len(ins):6d} {sum(s.startswith('s_cbranch') for s in ins):7d} {lp[0]:>9d}/{lp[1]}/{lp[2]:<7d}  {txt}")


if __name__ == "__main__":
    main()
