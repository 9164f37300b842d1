"""Every kernel of two builds side by side: the figures of hipcc's
-Rpass-analysis=kernel-resource-usage remarks (SGPRs, VGPRs, AGPRs, scratch,
spills, occupancy, LDS) from the two build logs, and the instruction count of
its disassembly with an instruction-for-instruction comparison
(kernel_diff.py) from the two libraries.  Build with `make -Otarget` so that
parallel jobs do not interleave their remarks.

    python scripts/isa/resource_table.py OLD_BUILD.log NEW_BUILD.log OLD.so NEW.so"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_diff as K  # noqa: E402

OLD_LOG, NEW_LOG, OLD_SO, NEW_SO = sys.argv[1:5]

def rows(log):
    cur, out = None, {}
    for ln in open(log, errors="replace"):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1); out.setdefault(cur, {}); continue
        m = re.search(r"remark:\s+(TotalSGPRs|SGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            out[cur][m.group(1)] = int(m.group(2))
    return out

def fmt(v):
    return "SGPR %3d VGPR %3d AGPR %d scratch %d B/lane spill %d/%d occupancy %d LDS %6d B" % (
        v.get("TotalSGPRs", v.get("SGPRs", -1)), v.get("VGPRs", -1), v.get("AGPRs", -1), v.get("ScratchSize [bytes/lane]", -1),
        v.get("SGPRs Spill", -1), v.get("VGPRs Spill", -1), v.get("Occupancy [waves/SIMD]", -1), v.get("LDS Size [bytes/block]", -1))

par, now = rows(OLD_LOG), rows(NEW_LOG)
names = sorted(set(par) | set(now))
dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()))
def short(n):
    d = dem[n]
    d = re.sub(r"^void ", "", d)
    d = re.sub(r"\(.*$", "", d)           # drop the argument list
    return d.replace("nice::fd2::", "").replace("nice::", "")
with tempfile.TemporaryDirectory() as tmp:
    ia = K.kernels(OLD_SO, tmp)
    ib = K.kernels(NEW_SO, tmp)
norm = lambda d: re.sub(r"\s+", "", K.key_of(d)).replace("(anonymousnamespace)", "")
ia = {norm(k): v for k, v in ia.items()}
ib = {norm(k): v for k, v in ib.items()}
def ninstr(tab, n):
    # kernel_diff keys: demangled names with argument lists
    d = norm(dem[n])
    return len(tab[d]) if d in tab else -1
same = diff = 0
lines_old, lines_new = [], []
for n in names:
    if n in par:
        a, b = par[n], now.get(n)
        d = norm(dem[n])
        ident = d in ia and d in ib and ia[d] == ib[d]
        ok = b is not None and a == b and ident
        same += ok; diff += (not ok)
        lines_old.append("%s\n    parent  %s  %6d instructions\n    now     %s  %6d instructions  %s" % (
            short(n), fmt(a), ninstr(ia, n), fmt(b) if b else "MISSING", ninstr(ib, n),
            "identical, instruction for instruction" if ok else "DIFFERS"))
    else:
        lines_new.append("%s\n    now     %s  %6d instructions" % (short(n), fmt(now[n]), ninstr(ib, n)))
print("existing kernels: %d, identical to the parent's (every resource figure and every instruction): %d, differing: %d" % (len(par), same, diff))
print("new kernels: %d, with scratch or spills: %d" % (len(lines_new), sum(1 for n in names if n not in par and (now[n].get("ScratchSize [bytes/lane]") or now[n].get("VGPRs Spill") or now[n].get("SGPRs Spill")))))
print("\n# --- new kernels ---")
print("\n".join(lines_new))
print("\n# --- existing kernels: parent and now ---")
print("\n".join(lines_old))
