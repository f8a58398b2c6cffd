#!/usr/bin/env python3
"""Per-kernel comparison of two builds' gfx950 device assembly.  No GPU, standard library only.

    python tools/isa_diff.py OLD_DIR NEW_DIR [--drop KERNEL:i,j ...] [--summary FILE]

OLD_DIR / NEW_DIR hold one .s file per translation unit (same file names on both sides), made with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -fuse-cuid=none [-x hip] UNIT -o UNIT.s
(`--emit DIR` does that for every unit of build.py's SOURCES of the tree this script sits in).

A refactor that must not change device code is checked kernel by kernel:
  identical    the instruction stream is the same, line for line (labels renumbered per kernel, comments dropped)
  normalised   the same after (a) every SGPR operand is rewritten to a placeholder and (b) s_load_* / s_mov_b32 / s_add*_i32 / s_cmp* lines are
               dropped - what a changed kernel-argument layout does to the scalar prologue; s_waitcnt, s_barrier, s_setprio, s_sleep, branches and
               everything non-scalar are kept
  DIFFERENT    anything else
and, for every matched pair, .vgpr_count, .agpr_count, .group_segment_fixed_size, .private_segment_fixed_size and .max_flat_workgroup_size of the
metadata must be present on both sides and equal (so no kernel gains scratch).  Kernels on one side only are listed as removed / added.

--drop KERNEL:i,j maps an OLD kernel to its NEW name by deleting the template arguments i, j (0-based) of the demangled name, for a refactor that
drops template parameters: --drop mlp_fused_lds_kernel:3,4.  Names are demangled with c++filt / llvm-cxxfilt.

Exit status 0: every matched kernel is identical or normalised, the metadata agree and nothing was added.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size")
SCALAR_DROP = re.compile(r"^(s_load_|s_mov_b32\b|s_add\w*_i32\b|s_cmp)")
SGPR = re.compile(r"\bs\[\d+:\d+\]|\bs\d+\b")


def find_cxxfilt():
    for name in ("c++filt", "llvm-cxxfilt"):
        p = shutil.which(name)
        if p:
            return p
    for root in (os.environ.get("ROCM_PATH", ""), "/opt/rocm"):
        p = os.path.join(root, "llvm", "bin", "llvm-cxxfilt")
        if root and os.path.exists(p):
            return p
    return None


def demangle(names):
    tool = find_cxxfilt()
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def split_template(name):
    """'void ns::k<a, b<c, d>, e>(args)' -> ('void ns::k', ['a', 'b<c, d>', 'e'], '(args)'); no template: (name, None, '')"""
    lt = name.find("<")
    if lt < 0:
        return name, None, ""
    depth, args, cur = 0, [], ""
    for i in range(lt, len(name)):
        ch = name[i]
        if ch in "<(":
            depth += 1
            if depth == 1:
                continue
        elif ch in ">)":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return name[:lt], args, name[i + 1:]
        elif ch == "," and depth == 1:
            args.append(cur.strip()); cur = ""
            continue
        cur += ch
    return name, None, ""


def apply_drop(name, drops):
    head, args, tail = split_template(name)
    if args is None:
        return name
    base = head.split("::")[-1].split()[-1]
    idx = drops.get(base)
    if not idx:
        return name
    return head + "<" + ", ".join(a for i, a in enumerate(args) if i not in idx) + ">" + tail


def parse_unit(path):
    """-> {mangled name: {'code': [instruction lines], 'meta': {key: value}}}"""
    lines = open(path, errors="replace").read().splitlines()
    kernels = {}
    names = set()
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            names.add(m.group(1))
    cur = None
    for ln in lines:
        s = ln.split(";", 1)[0].strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur = s[:-1]; kernels[cur] = {"code": [], "meta": {}}
            continue
        if re.match(r"\.Lfunc_end\d+:", s):
            cur = None
            continue
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        kernels[cur]["code"].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
    # metadata: the YAML list under amdhsa.kernels.  Only '  - ' at the list's own indentation opens a kernel entry and only keys at that entry's
    # indentation belong to the kernel: the nested '.args:' list has '- ' items and keys of its own, further in.
    entry, inside = None, False
    def close(e):
        if e and e.get(".name") in kernels:
            kernels[e[".name"]]["meta"] = e
    for ln in lines:
        if not ln.startswith(" "):
            close(entry); entry = None
            inside = ln.startswith("amdhsa.kernels:")
            continue
        if not inside:
            continue
        m = re.match(r"  (- | {2})(\.\w+):\s*(\S.*)?$", ln)
        if not m:
            continue
        if m.group(1) == "- ":
            close(entry); entry = {}
        if entry is not None and m.group(3) is not None:
            entry[m.group(2)] = m.group(3).strip().strip("'")
    close(entry)
    return kernels


def normalise(code):
    out = []
    for s in code:
        if SCALAR_DROP.match(s):
            continue
        out.append(SGPR.sub("s#", s))
    return out


def compare_units(old_path, new_path, drops):
    old, new = parse_unit(old_path), parse_unit(new_path)
    dm_old, dm_new = demangle(sorted(old)), demangle(sorted(new))
    new_by_name = {dm_new[k]: k for k in new}
    res = {"identical": [], "normalised": [], "different": [], "removed": [], "added": [], "meta": []}
    matched = set()
    for k in sorted(old, key=lambda k: dm_old[k]):
        want = apply_drop(dm_old[k], drops)
        nk = new_by_name.get(want)
        if nk is None:
            res["removed"].append(dm_old[k]); continue
        matched.add(nk)
        a, b = old[k], new[nk]
        bad = [f"{key}: {a['meta'].get(key, 'MISSING')} -> {b['meta'].get(key, 'MISSING')}" for key in META_KEYS
               if key not in a["meta"] or key not in b["meta"] or a["meta"][key] != b["meta"][key]]     # a value that was not found on either side is a mismatch, never a pass
        if bad:
            res["meta"].append(f"{want}: " + ", ".join(bad))
        if a["code"] == b["code"]:
            res["identical"].append(want)
        elif normalise(a["code"]) == normalise(b["code"]):
            res["normalised"].append(want)
        else:
            res["different"].append(want)
    res["added"] = sorted(dm_new[k] for k in new if k not in matched)
    res["n_old"], res["n_new"] = len(old), len(new)
    return res


def emit(out_dir):
    """device assembly of every unit of build.py's SOURCES (same flags as the product build)"""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(here, "..", "efficient-speech-codec_amd")
    sys.path.insert(0, pkg)
    import build as b
    os.makedirs(out_dir, exist_ok=True)
    procs = []
    for src in b.SOURCES:
        cmd = [b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-S", "-fuse-cuid=none"] + (["-x", "hip"] if src.endswith(".cpp") else []) + \
              [os.path.join(b.CSRC, src), "-o", os.path.join(out_dir, src + ".s")]
        procs.append((src, subprocess.Popen(cmd)))
    bad = [src for src, p in procs if p.wait() != 0]
    if bad:
        sys.exit("hipcc failed for " + ", ".join(bad))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_dir", nargs="?"); ap.add_argument("new_dir", nargs="?")
    ap.add_argument("--drop", action="append", default=[], metavar="KERNEL:i,j")
    ap.add_argument("--summary", metavar="FILE")
    ap.add_argument("--emit", metavar="DIR", help="write the .s files of this tree to DIR and exit")
    a = ap.parse_args()
    if a.emit:
        emit(a.emit); return 0
    if not a.old_dir or not a.new_dir:
        ap.error("OLD_DIR and NEW_DIR are required")
    drops = {}
    for d in a.drop:
        name, idx = d.split(":")
        drops[name] = {int(i) for i in idx.split(",")}
    units = sorted(f for f in os.listdir(a.old_dir) if f.endswith(".s"))
    missing = [u for u in units if not os.path.exists(os.path.join(a.new_dir, u))]
    if missing:
        sys.exit("units missing from " + a.new_dir + ": " + ", ".join(missing))
    lines, tot, ok = [], {k: 0 for k in ("n_old", "n_new", "identical", "normalised", "different", "removed", "added", "meta")}, True
    detail = {"normalised": [], "different": [], "removed": [], "added": [], "meta": []}
    for u in units:
        r = compare_units(os.path.join(a.old_dir, u), os.path.join(a.new_dir, u), drops)
        lines.append(f"{u}: {r['n_old']} -> {r['n_new']} kernels; identical {len(r['identical'])}, normalised {len(r['normalised'])}, "
                     f"DIFFERENT {len(r['different'])}, removed {len(r['removed'])}, added {len(r['added'])}, metadata mismatches {len(r['meta'])}")
        for k in tot:
            tot[k] += r[k] if isinstance(r[k], int) else len(r[k])
        for k in detail:
            detail[k] += [f"{u}: {n}" for n in r[k]]
        ok = ok and not r["different"] and not r["added"] and not r["meta"]
    lines.append(f"total: {tot['n_old']} -> {tot['n_new']} kernels; identical {tot['identical']}, normalised {tot['normalised']}, DIFFERENT {tot['different']}, "
                 f"removed {tot['removed']}, added {tot['added']}, metadata mismatches {tot['meta']}")
    for k, title in (("different", "DIFFERENT beyond the normalisation"), ("meta", "metadata mismatches"), ("added", "only in the new build"),
                     ("removed", "only in the old build"), ("normalised", "equal after normalisation")):
        if detail[k]:
            lines.append(""); lines.append(f"{title} ({len(detail[k])}):")
            lines += ["  " + n for n in detail[k]]
    lines.append(""); lines.append("verdict: " + ("PASS" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.summary:
        open(a.summary, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
