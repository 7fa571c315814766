"""Kernel names and resources of every .hip under a csrc directory, for comparing two trees (a refactor must change neither).

    python scripts/kernel_resources.py CSRC_DIR SUMMARY.txt [FULL.txt]

Compiles each source with the product flags plus -Rpass-analysis=kernel-resource-usage.  FULL.txt gets one line per kernel
(source, demangled name, SGPRs, VGPRs, AGPRs, scratch, dynamic stack, occupancy, spills, LDS), sorted.  SUMMARY.txt gets one line per
(source, kernel template): the number of instantiations, the ranges of the figures and a SHA-256 over the template's full lines --
equal summaries mean equal name sets and equal figures for every kernel; where a hash differs, diff the two FULL.txt."""
import hashlib, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result", "-Wno-unused-value",
         "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]"]


def kernels(csrc, src):
    r = subprocess.run(["hipcc"] + FLAGS + [src], cwd=csrc, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = []
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*)\[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            rows.append({"name": t.split(":", 1)[1].strip()})
        elif rows and ":" in t:
            k, v = t.rsplit(":", 1)
            rows[-1][k.strip()] = v.strip()
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    return [(src, n, [r.get(k, "?") for k in KEYS]) for r, n in zip(rows, names)]


def main(csrc, summary, full=None):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(4) as ex:
        rows = sorted(k for ks in ex.map(lambda s: kernels(csrc, s), srcs) for k in ks)
    short = [k.split(" [")[0].replace(" ", "") for k in KEYS]
    lines = ["%s | %s | %s" % (s, n, " ".join("%s=%s" % kv for kv in zip(short, v))) for s, n, v in rows]
    if full:
        open(full, "w").write("\n".join(lines) + "\n")
    groups = {}
    for (s, n, v), line in zip(rows, lines):
        groups.setdefault((s, re.sub(r"^void ", "", n).split("<")[0].split("(")[0]), []).append((v, line))
    rng = lambda g, i: "%d..%d" % (min(int(v[i]) for v, _ in g), max(int(v[i]) for v, _ in g))
    out = ["%s | %s | kernels=%d SGPRs=%s VGPRs=%s scratch=%s occupancy=%s LDS=%s sha256=%s"
           % (s, t, len(g), rng(g, 0), rng(g, 1), rng(g, 3), rng(g, 5), rng(g, 8), hashlib.sha256("\n".join(l for _, l in g).encode()).hexdigest()[:16])
           for (s, t), g in sorted(groups.items())]
    out.append("total | kernels=%d sha256=%s" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))
    open(summary, "w").write("\n".join(out) + "\n")
    print(len(lines), "kernels,", len(groups), "templates")


if __name__ == "__main__":
    main(*sys.argv[1:4])
