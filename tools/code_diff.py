"""Do two builds of the library hold the same device code for a set of kernels?  python tools/code_diff.py LIB_A LIB_B [substring of the mangled names, default bcsc_]
Compares, symbol by symbol, the instruction lists dma_wait_scan.bodies disassembles from each library's gfx950 code objects (no GPU needed) and prints the counts;
the exit status is the number of symbols that differ or exist on one side only.  A symbol's list ends at its last s_endpgm: what the disassembler shows behind it
(s_nop 0, or "..." for zero bytes) is the fill up to the next symbol's alignment, which depends on the symbol's place in the section; the count of symbols whose
fill differs is printed too."""
import sys
import dma_wait_scan as dws


def body(ins):
    end = len(ins)
    while end and ins[end - 1] in ("s_nop 0", "..."):
        end -= 1
    return ins[:end] if end and ins[end - 1] == "s_endpgm" else ins


if __name__ == "__main__":
    key = sys.argv[3] if len(sys.argv) > 3 else "bcsc_"
    a, b = ({n: ins for n, ins in dws.bodies(lib) if key in n} for lib in sys.argv[1:3])
    names = sorted(set(a) | set(b))
    differing = [n for n in names if n not in a or n not in b or body(a[n]) != body(b[n])]
    fill = [n for n in names if n not in differing and a[n] != b[n]]
    for n in differing:
        print("differs" if n in a and n in b else "on one side only", n)
    print(f"symbols compared {len(names)}, instructions {sum(len(body(x)) for x in a.values())} / {sum(len(body(x)) for x in b.values())}, "
          f"symbols differing {len(differing)} (fill behind the last s_endpgm differs for {len(fill)})")
    sys.exit(len(differing))
