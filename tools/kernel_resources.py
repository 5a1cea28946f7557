"""Per-kernel register / LDS / scratch use from a build log made with -Rpass-analysis=kernel-resource-usage, and the difference
between two such logs (a change that adds kernel variants must leave every existing kernel's figures as they were):

    make -C pointcloudprocessing_amd/csrc clean
    make -C pointcloudprocessing_amd/csrc CXXFLAGS='... -Rpass-analysis=kernel-resource-usage' 2> new.log
    python tools/kernel_resources.py new.log              # table; exit status 1 if any kernel spills to scratch
    python tools/kernel_resources.py old.log new.log      # kernels that appeared, disappeared or changed
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"), ("LDS Size [bytes/block]", "lds"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except Exception:
        return {n: n for n in names}


def row(d):
    return " ".join(f"{k}={d.get(k, '?')}" for _, k in FIELDS)


def main():
    if len(sys.argv) == 2:
        k = parse(sys.argv[1])
        names = demangle(sorted(k))
        bad = 0
        for n in sorted(k):
            print(f"{row(k[n])}  {names[n][:160]}")
            bad += 1 if (k[n].get("scratch", 0) or k[n].get("vspill", 0)) else 0
        print(f"{len(k)} kernels, {bad} with scratch or spilled vector registers")
        return 1 if bad else 0
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(old) | set(new)))
    changed = 0
    for n in sorted(set(old) | set(new)):
        if n not in old:
            print(f"NEW      {row(new[n])}  {names[n][:160]}")
        elif n not in new:
            print(f"GONE     {row(old[n])}  {names[n][:160]}")
            changed += 1
        elif old[n] != new[n]:
            print(f"CHANGED  {row(old[n])} -> {row(new[n])}  {names[n][:160]}")
            changed += 1
    print(f"{len(old)} kernels before, {len(new)} after, {changed} existing kernels changed or gone")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
