"""python tools/dbg/code_object_digest.py CSRC_DIR [--define NAME[=V] ...] [--only FILE.hip ...] [--stamp-builds] [--out FILE.json]
python tools/dbg/code_object_digest.py --compare PARENT.json THIS.json [--out FILE.json]
Device code of every file in the Makefile's SRC, compiled for the device alone with the Makefile's CXXFLAGS:
sha256 of the raw .text and .rodata bytes and, per kernel, the resource figures of the code object's notes, as
{build label: {"flags", "files"}}; --stamp-builds adds the two diagnostic builds, each on its kernel's file.
Two trees whose outputs are equal ship the same device code (whole-file hashes differ between two builds of
one tree; these do not).  --compare puts two such outputs into one file, with `equal` per build and file, and
exits 1 if anything differs.  Needs no GPU.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
STAMP_BUILDS = [("bm_kernels.hip", "EXABM4D_BM_STAMPS"), ("stage_kernels.hip", "EXABM4D_STAMPS")]
FIELDS = {
    "vgpr": ".vgpr_count", "agpr": ".agpr_count", "sgpr": ".sgpr_count", "vgpr_spill": ".vgpr_spill_count",
    "sgpr_spill": ".sgpr_spill_count", "scratch": ".private_segment_fixed_size", "lds": ".group_segment_fixed_size",
}


def make_var(text, name):
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M)
    return m.group(1).strip()


def section_digest(obj, section, tmp):
    raw = os.path.join(tmp, "section.bin")
    if os.path.exists(raw):
        os.remove(raw)
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={section}", obj, raw], check=True)
    data = open(raw, "rb").read() if os.path.exists(raw) else b""
    return {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def kernels(obj):
    notes = subprocess.run([f"{LLVM}/llvm-readobj", "--notes", obj], check=True, capture_output=True, text=True).stdout
    out = {}
    if "amdhsa.kernels:" not in notes:                          # a host-only file
        return out
    listed = re.split(r"^\S", notes.split("amdhsa.kernels:", 1)[1], 1, flags=re.M)[0]    # up to the next top-level key
    for block in re.split(r"^  - ", listed, flags=re.M)[1:]:
        top = dict(re.findall(r"^(?:    )?(\.[a-z_]+):\s*(\S+)\s*$", block, re.M))   # a kernel's own fields: indent 4 (0 on its first line)
        out[top[".name"]] = {short: int(top[field]) for short, field in FIELDS.items() if field in top}
    return {k: out[k] for k in sorted(out)}


def digest(csrc, defines, only):
    mk = open(os.path.join(csrc, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", make_var(mk, "HIPCC"))
    flags = make_var(mk, "CXXFLAGS").replace("$(ARCH)", make_var(mk, "ARCH")).split()
    flags += ["-D" + d for d in defines] + ["--cuda-device-only", "--no-gpu-bundle-output", "-c"]
    res = {"flags": " ".join(flags), "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for src in only or make_var(mk, "SRC").split():
            obj = os.path.join(tmp, src + ".co")
            subprocess.run([hipcc, *flags, src, "-o", obj], check=True, cwd=csrc)
            res["files"][src] = {"text": section_digest(obj, ".text", tmp), "rodata": section_digest(obj, ".rodata", tmp),
                                 "kernels": kernels(obj)}
            print(src, res["files"][src]["text"]["sha256"][:16], len(res["files"][src]["kernels"]), "kernels", file=sys.stderr)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csrc", nargs="?")
    ap.add_argument("--define", action="append", default=[])
    ap.add_argument("--only", action="append", default=[])
    ap.add_argument("--stamp-builds", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT.json", "THIS.json"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.compare:
        parent, this = (json.load(open(f)) for f in a.compare)
        equal = {b: {f: parent[b]["files"].get(f) == this[b]["files"].get(f)
                     for f in sorted(set(parent[b]["files"]) | set(this[b]["files"]))} for b in parent}
        res = {"equal": equal, "parent": parent, "this": this}
        same = set(parent) == set(this) and all(all(e.values()) for e in equal.values())
    else:
        label = " ".join(a.only + ["-D" + d for d in a.define]) or "default"
        res = {label: digest(a.csrc, a.define, a.only)}
        if a.stamp_builds:
            for src, d in STAMP_BUILDS:
                res[f"{src} -D{d}"] = digest(a.csrc, a.define + [d], [src])
        same = True
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        open(a.out, "w").write(text + "\n")
    else:
        print(text)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
