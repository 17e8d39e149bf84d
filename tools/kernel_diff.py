#!/usr/bin/env python3
"""Compare the generated gfx950 code of two builds, kernel by kernel.

Each directory holds, per translation unit, NAME.s and NAME.remarks: the output and the stderr of
    hipcc $(HIPFLAGS) --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -x hip -c NAME.hip -o NAME.s
(HIPFLAGS as in the Makefile).  Prints the kernels whose resources or instruction streams differ and
the kernels only one side has.  Exit status 1 if a resource of any kernel rose (for occupancy: fell),
if the kernel sets or the units of the two directories differ, or if there is no unit at all; a
resource that only improved is listed and counted, and does not fail.

    tools/kernel_diff.py DIR_OLD DIR_NEW
"""
import re
import subprocess
import sys
from pathlib import Path

RESOURCES = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
             "VGPRs Spill", "LDS Size [bytes/block]")   # TotalSGPRs may move


def resources(path):
    out, cur = {}, None
    for line in path.read_text().splitlines():
        m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def streams(path):
    """function symbol -> its instructions and labels (comments, directives, __hip_cuid_* dropped)"""
    out, cur = {}, None
    for line in path.read_text().splitlines():
        line = line.split(";")[0].strip()
        if cur is None:
            m = re.fullmatch(r"(\w+):", line)
            if m and not m.group(1).startswith("__hip_cuid_"):
                cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif line.startswith("__hip_cuid_"):   # the unit's id, a hash of its source, after the last data symbol
            continue
        elif line and (not line.startswith(".") or line.endswith(":")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line))   # labels carry the function's number
    return out


def demangle(names):
    names = list(names)
    if not names:
        return {}
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, res.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(old, new):
    old, new = Path(old), Path(new)
    bad = False
    total = same = worse = better = 0
    units = {p.name for p in old.glob("*.s")} | {p.name for p in new.glob("*.s")}
    if not units:
        print("no NAME.s in either directory")
        return 1
    for unit in sorted(units):
        so, sn = old / unit, new / unit
        if not so.exists() or not sn.exists():
            print(f"{so.stem}: only in {'old' if so.exists() else 'new'}")
            bad = True
            continue
        ro, rn = resources(so.with_suffix(".remarks")), resources(sn.with_suffix(".remarks"))
        to, tn = streams(so), streams(sn)
        names = demangle(set(ro) | set(rn))
        changed = []
        for k in sorted(set(ro) | set(rn), key=names.get):
            if k not in ro or k not in rn:
                print(f"{so.stem}: only in {'old' if k in ro else 'new'}: {names[k]}")
                bad = True
                continue
            total += 1
            dr = [f"{r} {ro[k].get(r)} -> {rn[k].get(r)}" for r in RESOURCES if ro[k].get(r) != rn[k].get(r)]
            # more of anything is worse, except occupancy
            up = [r for r in RESOURCES if ro[k].get(r) != rn[k].get(r)
                  and (int(rn[k][r]) > int(ro[k][r])) != r.startswith("Occupancy")]
            worse += bool(up)
            better += bool(dr) and not up
            if dr or to.get(k) != tn.get(k):
                sg = "" if ro[k].get("TotalSGPRs") == rn[k].get("TotalSGPRs") else \
                    f"TotalSGPRs {ro[k].get('TotalSGPRs')} -> {rn[k].get('TotalSGPRs')}"
                changed.append(f"  {names[k]}: instructions {len(to.get(k, []))} -> {len(tn.get(k, []))}"
                               + "".join("; " + d for d in dr + ([sg] if sg else [])))
            else:
                same += 1
        # device functions the kernels call (not inlined) are part of their streams
        for k in sorted((set(to) | set(tn)) - set(ro) - set(rn)):
            if to.get(k) != tn.get(k):
                changed.append(f"  (device function) {k}: instructions {len(to.get(k, []))} -> {len(tn.get(k, []))}")
        print(f"{so.stem}: {len(ro)} kernels, {len(changed)} changed")
        print("\n".join(changed), end="\n" if changed else "")
    print(f"total: {total} kernels in both, {same} identical; resources worse in {worse}, better only in {better}"
          + ("; kernel sets or units differ" if bad else ""))
    return 1 if bad or worse else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
