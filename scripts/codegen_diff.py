#!/usr/bin/env python
"""Compare the device assembly of two builds symbol by symbol.

    hipcc <edgerunner_amd.build.FLAGS without -shared -fPIC> --cuda-device-only -S -o parent.s er_api.hip    (in the parent's csrc)
    hipcc ... -o new.s er_api.hip                                                                            (in this tree's csrc)
    python scripts/codegen_diff.py parent.s new.s > profiles/<name>_codegen.log

A symbol is its instruction stream plus its kernel descriptor (.amdhsa_* block).  Basic-block and function-end labels carry the
function's ordinal in the file, which shifts when kernels are added, so `.LBB<n>_` / `.Lfunc_end<n>` and the `BB<n>_` of the loop
comments are compared without the ordinal.
Exit status 1 when a symbol of the first file is missing from or differs in the second."""
import re
import sys


def symbols(path):
    text = open(path).read()
    out = {}
    for name, body in re.findall(r"\n(_Z[^\n:]*):\s*; @[^\n]*\n(.*?\n\.Lfunc_end\d+:)", text, flags=re.S):
        out[name] = body
    for name, desc in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        if name in out:
            out[name] += "\n" + desc
    # (a label's ordinal also sets the width of the padding in front of its comment)
    norm = lambda b: re.sub(r"[ \t]+", " ", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", re.sub(r"\bBB\d+_", "BB_", re.sub(r"\.LBB\d+_", ".LBB_", b))))
    return {n: norm(b) for n, b in out.items()}


def main():
    old, new = symbols(sys.argv[1]), symbols(sys.argv[2])
    missing = sorted(n for n in old if n not in new)
    changed = sorted(n for n in old if n in new and old[n] != new[n])
    added = sorted(n for n in new if n not in old)
    print(f"symbols in the parent build: {len(old)}")
    print(f"identical in this build (instructions and kernel descriptor): {len(old) - len(missing) - len(changed)}")
    print(f"changed: {len(changed)}")
    for n in changed:
        print("  " + n)
    print(f"missing: {len(missing)}")
    for n in missing:
        print("  " + n)
    print(f"added: {len(added)}")
    for n in added:
        b = new[n]
        ins = [l.strip() for l in b.split("\n") if l.strip() and not l.strip().startswith((";", "."))]
        vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", b)
        scratch = sum(l.startswith("scratch_") for l in ins)
        print(f"  {n}: {len(ins)} instructions, vgpr {vg.group(1) if vg else '?'}, scratch accesses {scratch}, "
              f"v_cvt_pk_f32_fp8 {sum('v_cvt_pk_f32_fp8' in l for l in ins)}, ds_bpermute {sum('ds_bpermute' in l for l in ins)}, "
              f"nt dwordx2 loads {sum(l.startswith('global_load_dwordx2') and l.endswith(' nt') for l in ins)}, "
              f"v_cvt_scalef32_pk_f32_fp4 {sum('v_cvt_scalef32_pk_f32_fp4' in l for l in ins)}, "
              f"nt dwordx4 loads {sum(l.startswith('global_load_dwordx4') and l.endswith(' nt') for l in ins)}")
    return 1 if (changed or missing) else 0


if __name__ == "__main__":
    sys.exit(main())
