"""Function-by-function comparison of two device assembly files of one translation unit, for refactors that must leave
kernels as they are.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S sf_fill.hip -o new.s   (per tree)
    python tools/asm_diff.py old.s new.s [name-part ...]
Per kernel: identical instruction stream or not (comments dropped, basic-block labels and the kernel's own symbol
normalised; the mangled names of argument structs may differ between the files), and for the kernels that differ, exist on
one side only or contain one of the name parts: VGPRs, occupancy, LDS bytes and scratch bytes of both sides.  A kernel whose
instructions are the same and whose descriptor directives alone moved (.amdhsa_kernarg_size of an argument struct that grew)
is reported as such, with the directives."""
import re
import sys


def kernels(path):
    """name -> (instruction lines, resource figures) of every function of the file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=; -- Begin function|\Z)", text, re.S | re.M):
        name, body, tail = m.groups()
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()).replace(name, "SELF") for ln in body.splitlines()]
        figures = {k: int(v) for k, v in re.findall(r"; (NumVgprs|Occupancy|LDSByteSize|ScratchSize): (\d+)", tail)}
        out[name] = ([ln for ln in lines if ln], figures)
    return out


def key(name):
    return re.sub(r"\d+sf_\w+", "ARGS", name)  # (the struct a kernel takes may have been renamed)


old, new = ({key(k): (k, *v) for k, v in kernels(p).items()} for p in sys.argv[1:3])
same = 0
for k in sorted(set(old) | set(new)):
    a, b = old.get(k), new.get(k)
    equal = a is not None and b is not None and a[1] == b[1]
    same += equal
    if not equal or any(part in k for part in sys.argv[3:]):
        state = "identical" if equal else "differs" if a and b else "only in " + (sys.argv[1] if a else sys.argv[2])
        if a and b and not equal:  # (the kernel descriptor's directives sit inside the function: an argument struct that grew)
            code = [[ln for ln in side[1] if not ln.startswith(".amdhsa_")] for side in (a, b)]
            if code[0] == code[1]:
                moved = sorted(set(a[1]) ^ set(b[1]))
                state = f"identical instructions, descriptor directives differ ({', '.join(moved)})"
        print(f"{(a or b)[0]}: {state}; {a[2] if a else '-'} -> {b[2] if b else '-'}")
print(f"{same} kernels with identical instruction streams, {len(set(old) | set(new)) - same} differ or exist on one side only")
