"""Compare the kernels of two device assembly listings (hipcc -S --offload-device-only of
madpose_amd/csrc/kernels/kernels.hip at two commits), without a device: per kernel the FP64
instruction multiset, the whole instruction multiset, VGPRs, SGPRs, scratch and LDS -- the check
that a change left the existing kernels' code objects alone.

    python tools/asm_compare.py parent.s this.s

Prints every kernel present in both whose FP64 multiset or resources differ, a summary line, and
the resources of the kernels only the second listing has.  Exit status 1 when a shared kernel
differs or one is missing."""
import collections
import re
import subprocess
import sys


def kernels(path):
    s = open(path).read()
    ms = list(re.finditer(r"^(_Z\S+):\s*;", s, re.M))
    out = {}
    for i, m in enumerate(ms):
        body = s[m.start(): ms[i + 1].start() if i + 1 < len(ms) else len(s)]
        if ".amdhsa_kernel" not in body and "s_endpgm" not in body:
            continue
        fp64 = collections.Counter(re.findall(r"^\s+(v_\w*f64\w*)", body, re.M))
        every = collections.Counter(re.findall(r"^\s+((?:[sv]|ds|global|buffer|flat|scratch)_\w+)", body, re.M))
        field = lambda k: (re.search(r"\.amdhsa_" + k + r" (\d+)", body) or [None, "?"])[1]
        out[m.group(1)] = (fp64, (field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"),
                                  field("group_segment_fixed_size")), every)
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    same = fp = res = whole = 0
    for k in a:
        if k not in b:
            continue
        if a[k][0] != b[k][0]:
            fp += 1
            print("FP64 multiset differs:", k)
        elif a[k][1] != b[k][1]:
            res += 1
            print("resources differ:", k, a[k][1], b[k][1])
        else:
            same += 1
        whole += a[k][2] != b[k][2]
    missing = [k for k in a if k not in b]
    print(f"kernels: {len(a)} in the first listing, {len(b)} in the second; shared with equal FP64 multiset, VGPRs, "
          f"SGPRs, scratch and LDS: {same}; FP64 multiset differs: {fp}; resources differ: {res}; whole instruction "
          f"multiset differs: {whole}; missing from the second: {len(missing)}")
    new = [k for k in b if k not in a]
    names = subprocess.run(["c++filt"], input="\n".join(new), capture_output=True, text=True).stdout.split("\n")
    for k, name in zip(new, names):
        short = re.sub(r"\(.*", "", name.replace("mp::(anonymous namespace)::", "")).replace("void ", "")
        v, sg, sc, lds = b[k][1]
        print(f"new: {short:28s} fp64 instructions {sum(b[k][0].values()):4d}  vgpr {v:>4s}  sgpr {sg:>4s}  scratch {sc}"
              f"  lds {lds}")
    return 1 if fp or res or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
