"""Compare the gfx950 code of every kernel of two device-only assembly builds (hipcc --cuda-device-only -S, one .s per translation
unit): per kernel, the instruction stream with comments and branch-target labels masked, and the registers / scratch / occupancy
of its metadata.  A kernel that moved to another translation unit is matched by its mangled name across the units of OLD_DIR.
Usage: isa_compare.py OLD_DIR NEW_DIR  (prints one line per kernel; kernels only in NEW_DIR are listed as new)."""
import os
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    text = open(path).read()
    bodies, meta = {}, {}
    for m in re.finditer(r"^([A-Za-z_]\w*):[ \t]*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name = m.group(1)
        if name.startswith("."):
            continue
        lines = []
        for ln in m.group(2).split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") and ln.endswith(":"):
                continue
            ln = re.sub(r"\.LBB\d+_\d+", ".LBB", ln)
            if ln.startswith(".") and not ln.startswith(".LBB"):
                continue                    # assembler directives (cfi, p2align)
            lines.append(ln)
        bodies[name] = lines
    for blk in re.split(r"\n  - \.", text.split("amdhsa.kernels:")[-1]):
        n = re.search(r"\.name:\s+(\S+)", blk)
        if not n:
            continue
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        meta[n.group(1)] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("agpr_count"))
    return {k: (bodies.get(k, []), v) for k, v in meta.items()}


def occupancy(vgpr, agpr):
    try:
        total = int(vgpr) + int(agpr if agpr != "?" else 0)
    except ValueError:
        return "?"
    granule = 8
    regs = -(-max(total, 1) // granule) * granule
    return str(min(8, 512 // regs))


def main(old_dir, new_dir):
    rows = []
    old_units = {f[:-2]: kernels(os.path.join(old_dir, f)) for f in sorted(os.listdir(old_dir)) if f.endswith(".s")}
    new_units = {f[:-2]: kernels(os.path.join(new_dir, f)) for f in sorted(os.listdir(new_dir)) if f.endswith(".s")}
    elsewhere = lambda units, tu, k: next((v[k] for u, v in units.items() if u != tu and k in v), None)
    for tu, new in new_units.items():
        # the unit's own kernels of OLD_DIR, and -- by mangled name -- the ones that came here from another unit
        old = dict(old_units.get(tu, {}))
        old.update({k: elsewhere(old_units, tu, k) for k in new if k not in old and elsewhere(old_units, tu, k)})
        names = demangle(list(new))
        for k, (body, (v, s, p, a)) in sorted(new.items(), key=lambda kv: (kv[0] not in old, names[kv[0]])):
            if k in old:
                state = "identical" if old[k][0] == body and old[k][1] == new[k][1] else "CHANGED"
            else:
                state = "new"
            rows.append((tu, names[k], state, len(body), v, s, p, occupancy(v, a)))
        for k in old:
            if k not in new and not elsewhere(new_units, tu, k):
                rows.append((tu, demangle([k])[k], "MISSING", 0, "-", "-", "-", "-"))
    for tu, old in old_units.items():           # a unit that is gone: what it held and no unit holds now
        if tu not in new_units:
            rows += [(tu, demangle([k])[k], "MISSING", 0, "-", "-", "-", "-") for k in old if not elsewhere(new_units, tu, k)]
    print(f"{'translation unit':22} {'kernel':70} {'code':10} {'instructions':>12} {'vgpr':>5} {'sgpr':>5} {'scratch':>8} {'occ':>4}")
    for r in rows:
        print(f"{r[0]:22} {r[1][:70]:70} {r[2]:10} {r[3]:12} {r[4]:>5} {r[5]:>5} {r[6]:>8} {r[7]:>4}")
    return 1 if any(r[2] in ("CHANGED", "MISSING") for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
