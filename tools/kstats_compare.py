"""Compare the kernels of two builds symbol by symbol: VGPRs, SGPRs, LDS, private segment (the code object's
metadata, as tools/kstats.py reads it) and code size (the function symbol's size). Prints one JSON object: the kernels
of the old build matching the regex, those whose figures differ in the new build, and the kernels only the new build has.
usage: python tools/kstats_compare.py old.so new.so [kernel-regex]"""
import json
import re
import subprocess
import sys
import tempfile

from kstats import code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def kernels(path, pat):
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
            syms = subprocess.run([READELF, "--symbols", "--wide", f.name], capture_output=True, text=True).stdout
        size = {}
        for ln in syms.splitlines():
            p = ln.split()
            if len(p) >= 8 and p[3] == "FUNC":
                size[p[7]] = int(p[2], 0)
        for blk in re.split(r"\n\s+- \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m or not pat.search(m.group(1)) or ".vgpr_count" not in blk:
                continue
            rec = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in KEYS if re.search(r"\." + k + r":", blk)}
            rec["code_bytes"] = size.get(m.group(1), -1)
            out[m.group(1)] = rec
    return out


def main():
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else r"ibl\d+(fl|ib)_")
    old, new = kernels(sys.argv[1], pat), kernels(sys.argv[2], pat)
    res = {"regex": pat.pattern, "old_kernels": len(old), "new_kernels": len(new),
           "missing_in_new": sorted(set(old) - set(new)),
           "changed": {k: {"old": old[k], "new": new[k]} for k in sorted(old) if k in new and old[k] != new[k]},
           "only_in_new": {k: new[k] for k in sorted(set(new) - set(old))}}
    res["identical"] = not res["missing_in_new"] and not res["changed"]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
