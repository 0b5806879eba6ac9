"""Build the native library in-tree: crowdnav_dsrnn_amd/lib/libcrowdnav_hip.so (gfx950).

Provenance: the library embeds `CN_SRC_HASH=<sha256 of the compile flags + every source it depends on>`
(returned by cn_version()). `_lib.lib()` refuses a library whose embedded hash differs from the hash of
the sources on disk, so a stale prebuilt binary can never stand in for the committed code.

This module is the ONE place that knows the compile recipe (compile_cmd). The diagnostic builds go through
it too -- extra defines, another output path, a hash tag, the sources of another tree, the per-kernel
resource report -- by `build_library()` / `resources()` or the command line (`python -m
crowdnav_dsrnn_amd.build --help`); the scripts under tools/ are wrappers around that command line.
"""
import argparse
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libcrowdnav_hip.so")
PKG = os.path.basename(HERE)


def sources(root=REPO):
    return [os.path.join(root, PKG, "csrc", n) for n in ("cn_engine.hip", "cn_gru.hip", "cn_attn_mask.hip", "cn_lattice.hip")]


def deps(root=REPO):
    """The sources, then every header under csrc/ (recursively) and include/, sorted: a header that exists is
    hashed, so none can be forgotten."""
    hdrs = glob.glob(os.path.join(root, PKG, "csrc", "**", "*.h"), recursive=True)
    hdrs += glob.glob(os.path.join(root, "include", "*.h"))
    return sources(root) + sorted(hdrs)


SOURCES = sources()
DEPS = deps()
ARCH = os.environ.get("CN_OFFLOAD_ARCH", "gfx950")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result"]
# Per-source extra flags. The step kernel's RNG phase inlines ocml's sin / cos / acos: machine LICM hoists
# their f64 polynomial constants (and kernel-argument copies) to the RNG loop's preheader, where they hold
# ~40 VGPRs across the whole loop; at the 3-workgroups-per-CU cap (168 VGPRs) that forced 34 VGPRs of
# scratch spills whose stores reached HBM every launch (~5 MB per C2 launch). Without machine LICM the C2
# variant fits in 165 VGPRs with no spill and the kd-tree variant drops 212 -> 178 VGPRs. The GRU
# kernels keep the default pipeline.
SRC_FLAGS = {"cn_engine.hip": ["-mllvm", "-disable-machine-licm"]}
HASH_MARK = b"CN_SRC_HASH="


def compile_cmd(src, defines=(), extra=()):
    """THE compile recipe of one source: arch, common flags, the source's own flags, then `defines` (for every
    source: '-DNAME[=V]'; for one: '-Dcn_gru.hip:NAME[=V]') and `extra`."""
    name = os.path.basename(src)
    ds = []
    for d in defines:
        d = d[2:] if d.startswith("-D") else d
        only, sep, rest = d.partition(":")
        if not (sep and only.endswith(".hip")):
            ds.append("-D" + d)
        elif only == name:
            ds.append("-D" + rest)
    return [hipcc(), "--offload-arch=" + ARCH] + FLAGS + SRC_FLAGS.get(name, []) + ds + list(extra) + [src]


def source_hash(root=REPO):
    """sha256 over the target arch, the compile flags and the bytes of every dependency, in order."""
    h = hashlib.sha256()
    h.update(("%s|%s|%s|" % (ARCH, " ".join(FLAGS), sorted(SRC_FLAGS.items()))).encode())
    for d in deps(root):
        h.update(os.path.relpath(d, root).encode() + b"\0")
        with open(d, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()


def built_hash(path=LIB_PATH):
    """The source hash embedded in a built library (None if absent or unreadable)."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    i = blob.find(HASH_MARK)
    if i < 0:
        return None
    return blob[i + len(HASH_MARK):i + len(HASH_MARK) + 64].decode("ascii", "replace")


def needs_build():
    return built_hash() != source_hash()


def build_library(out=LIB_PATH, defines=(), tag=None, root=REPO, verbose=False):
    """Compile the sources under `root` and link them into `out`. The library embeds `tag`, or the source hash
    of `root`."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    tmp = out + ".tmp%d" % os.getpid()
    mark = '-DCN_SRC_HASH="%s"' % (tag or source_hash(root))
    objs = []
    try:
        procs = []
        for src in sources(root):   # one object per source (its own flags), compiled side by side, then one link
            obj = "%s.%s.o" % (tmp, os.path.basename(src))
            cmd = compile_cmd(src, defines, [mark, "-c", "-o", obj])
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((subprocess.Popen(cmd), cmd))
            objs.append(obj)
        failed = [cmd for p, cmd in procs if p.wait() != 0]
        if failed:
            raise subprocess.CalledProcessError(1, failed[0])
        cmd = [hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", tmp] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    finally:
        for o in objs:
            if os.path.exists(o):
                os.remove(o)
    os.replace(tmp, out)
    return out


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB_PATH
    return build_library(verbose=verbose)


RES_KEYS = ["VGPRs", "AGPRs", "SGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
            "Occupancy [waves/SIMD]"]


def resources(names=(), defines=(), root=REPO, file=sys.stdout):
    """Per-kernel register / spill / LDS / occupancy table of the sources (all, or those named): a device-only
    compile with the build's own flags per source and the compiler's kernel-resource-usage remarks. No GPU."""
    rows = []
    for src in sources(root):
        if names and os.path.basename(src) not in names:
            continue
        with tempfile.TemporaryDirectory() as t:
            cmd = compile_cmd(src, defines, ["-c", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                                             "-o", os.path.join(t, "res.o")])
            p = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if p.returncode:
            sys.stderr.write(p.stderr)
            raise subprocess.CalledProcessError(p.returncode, cmd)
        cur = None
        for l in p.stderr.splitlines():
            if "remark:" not in l:
                continue
            l = l.split("remark:", 1)[1].split(" [-Rpass")[0].strip()
            if l.startswith("Function Name:"):
                cur = {"name": l.split(":", 1)[1].strip()}
                rows.append(cur)
            elif cur is not None and ":" in l:
                k, v = l.split(":", 1)
                cur[k.strip()] = v.strip()
    print("%-48s" % "kernel" + "".join("%10s" % k.split()[0][:9] + ("sp" if "Spill" in k else "") for k in RES_KEYS),
          file=file)
    for r in rows:
        # (some compiler versions name the SGPR count "TotalSGPRs")
        print("%-48s" % r["name"][:48] + "".join("%10s" % r.get(k, r.get("Total" + k, "-")) for k in RES_KEYS), file=file)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m crowdnav_dsrnn_amd.build", description=__doc__.split("\n\n")[0])
    ap.add_argument("--force", action="store_true", help="rebuild even if the library matches the sources")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="[SOURCE:]NAME[=VALUE]",
                    help="extra define for every source, or for one (-Dcn_gru.hip:GF_WPC=3)")
    ap.add_argument("--out", default=None, help="output library (default: the in-tree library)")
    ap.add_argument("--tag", default=None, help="embed this as CN_SRC_HASH in place of the source hash")
    ap.add_argument("--root", default=REPO, help="build the sources of this tree (a checkout of another revision)")
    ap.add_argument("--resources", nargs="*", default=None, metavar="SOURCE",
                    help="no build: print the per-kernel resource table (of the named sources, default all)")
    a = ap.parse_args(argv)
    if a.resources is not None:
        resources(a.resources, a.defines, a.root)
        return 0
    if a.out is None and not (a.defines or a.tag or a.root != REPO):
        print(build(force=a.force, verbose=True))   # the shipped library
    else:
        if a.out is None:
            ap.error("a variant build (defines, --tag, --root) needs --out: the in-tree library is only ever "
                     "built from the tree as it is")
        print(build_library(a.out, a.defines, a.tag, a.root, verbose=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
