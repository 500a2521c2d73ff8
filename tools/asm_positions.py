"""Where a kernel's vector loads sit relative to its fp64 arithmetic, from hipcc's assembly
(``hipcc <flags> --cuda-device-only -S -o x.s x.hip``):

    python tools/asm_positions.py x.s adam_sum4_kernel adam_sum4_pair_kernel ...

Per kernel whose symbol contains one of the names: the instruction count, the number of fp64 VALU
instructions and the positions (0-based instruction index) of the first and last of them, of the first
vector memory load, of the first ``s_barrier`` and of the first vector store.
"""
import re
import sys


def kernels(path):
    name, body = None, []
    for line in open(path):
        s = line.strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):", s)
        if m and not s.startswith(".L"):
            if name:
                yield name, body
            name, body = m.group(1), []
        elif s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
            if name:
                yield name, body
            name, body = None, []
        elif name and s and not s.startswith((".", ";", "//")):
            body.append(s.split()[0])


def first(ops, pred):
    return next((i for i, o in enumerate(ops) if pred(o)), None)


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    for name, ops in kernels(path):
        if not any(w in name for w in wanted) or not ops:
            continue
        f64 = [i for i, o in enumerate(ops) if o.startswith("v_") and "f64" in o]
        load = first(ops, lambda o: o.startswith(("global_load", "buffer_load", "flat_load")))
        store = first(ops, lambda o: o.startswith(("global_store", "buffer_store", "flat_store")))
        bar = first(ops, lambda o: o == "s_barrier")
        print(f"{name}: {len(ops)} instructions, {len(f64)} fp64 VALU"
              + (f" at {f64[0]}..{f64[-1]}" if f64 else "")
              + f", first vector load at {load}, first s_barrier at {bar}, first vector store at {store}")


if __name__ == "__main__":
    main()
