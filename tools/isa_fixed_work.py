#!/usr/bin/env python
"""Static census of a render kernel's ISA BY REGION OF ITS SOURCE: how many instructions of each class a workgroup spends before
its first work item, once per tile (prologue, staging, masks + lists, write-out, epilogue) and in the walk.  The companion of
tools/isa_census.py (which counts per basic block); needs no GPU.

The translation unit is compiled with the project's own flags (topo4d_amd/build.py: FLAGS, plus T4D_CFLAGS) and
`-gline-tables-only -S --cuda-device-only`; line tables change no instruction.  Every instruction is attributed to the source line
of the KERNEL it was inlined into (the outermost entry of the location the compiler prints behind each `.loc`), and a line belongs
to the region named by the last `// T4D_REGION <name>` comment above it in the kernel's file.  Comments emit nothing.

Classes: vector (v_*), scalar (s_*), LDS (ds_*), memory (global / buffer / flat / scratch), lane (v_readlane / v_writelane: how
scalar registers are spilled) and f64 (v_*_f64); lane and f64 are also counted as vector.  Counts are STATIC: a loop's body counts
once (the dynamic figure is the GPU's SQ_INSTS_VALU), so what the table shows is which region changed and that the walk did not.
`walk_block` is the vector count of the walk's largest basic block: in the forward's throughput build that is the whole loop body,
four steps (89 = 4 x 22.25); the backward's four steps are separate blocks (a same-splat test between them), compare its walk row.

    python tools/isa_fixed_work.py 'k_render_bwdILb0ELb0ELi0ELb0E' 'k_render_fwdILb0ELi192ELi0ELb0ELb0E' [--root DIR] [--json OUT]
    python tools/isa_fixed_work.py ... --before OLD.json        # before / after table (markdown)

--dynamic LANES.jsonl adds, per kernel, a DYNAMIC estimate for the regions that run once per staged batch (staging, masks + lists,
write-out): every basic block's vector count x the block's trip count per launch, trip counts from the counted launch of
tools/count_lanes.py (profiles/r06_lanes.jsonl; --config / --opacity pick the record):
  masks + lists   a block runs once per live wave-batch (`wave_batches`); a block that branches to itself (the padding loops: 64
                  entries a trip) once as well;
  staging,        once per wave that holds a staged splat: sum over tiles of ceil(n / 64) ~ pairs / 64 + nonempty_tiles / 2;
  write-out       a block that branches to itself (the loop over the four waves' slabs) four times that.
An UPPER estimate: both arms of every wave-uniform branch and every tail-duplicated copy of a block are counted as if each ran;
what it is for is the DIFFERENCE between two trees, set against the difference SQ_INSTS_VALU measures.
"""
import argparse, json, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = ("vector", "scalar", "lds", "memory", "lane", "f64")


def compile_asm(root, out):
    sys.path.insert(0, os.path.dirname(HERE))
    from topo4d_amd import build as b
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + b.FLAGS + os.environ.get("T4D_CFLAGS", "").split() + \
          ["-gline-tables-only", "-S", "--cuda-device-only", os.path.join(root, "topo4d_amd", "csrc", "t4d_raster.hip"), "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def region_markers(path):
    """[(line, name)] of the `// T4D_REGION name` comments of a source file, ascending."""
    out = []
    for i, l in enumerate(open(path), 1):
        m = re.match(r"\s*// T4D_REGION (.+?)\s*$", l)
        if m:
            out.append((i, m.group(1)))
    return out


def classify(op):
    c = []
    if op.startswith("v_"):
        c.append("vector")
        if op.startswith(("v_readlane", "v_writelane")):
            c.append("lane")
        if "_f64" in op:
            c.append("f64")
    elif op.startswith("ds_"):
        c.append("lds")
    elif op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        c.append("memory")
    elif op.startswith("s_"):
        c.append("scalar")
    return c


def census(asm_lines, want, root, dump=None, lanes=None):
    start = next(i for i, l in enumerate(asm_lines) if re.match(r"^_Z\w*" + re.escape(want) + r"\w*:", l))
    end = next(i for i in range(start, len(asm_lines)) if asm_lines[i].startswith(".Lfunc_end"))
    name = asm_lines[start].split(":")[0]
    markers, order = {}, []          # file -> markers
    region = "entry"
    counts = {}
    new_block = lambda label: {"region": None, "vector": 0, "label": label, "by_region": {}, "loops": False}
    block, blocks = new_block(None), []
    for l in asm_lines[start + 1:end]:
        t = l.strip()
        if t.startswith(".loc"):
            locs = re.findall(r"([^\s\[\]@;]+):(\d+):\d+", t.split(";", 1)[1]) if ";" in t else []
            if locs:
                f, line = locs[-1][0], int(locs[-1][1])              # outermost: the kernel's own line
                if line > 0 and "t4d_raster_render" in f:
                    if f not in markers:
                        p = f if os.path.isabs(f) else os.path.join(root, f)
                        markers[f] = region_markers(p) if os.path.exists(p) else []
                    for ml, mn in markers[f]:
                        if ml <= line:
                            region = mn
            continue
        if re.match(r"^\.LBB\d+_\d+:", t):
            if dump:
                print(t.split(";")[0].strip())
            blocks.append(block)
            block = new_block(t.split(":")[0])
            continue
        if not t or t[0] in ";.":
            continue
        op = t.split()[0]
        if op.startswith("s_cbranch") and t.split()[1:2] == [block["label"]]:
            block["loops"] = True
        cl = classify(op)
        if not cl:
            continue
        if dump and region == dump:
            print("\t" + t.split(";")[0].strip())
        if region not in counts:
            counts[region] = dict.fromkeys(CLASSES, 0)
            order.append(region)
        for c in cl:
            counts[region][c] += 1
        if "vector" in cl:
            block["vector"] += 1
            block["region"] = block["region"] or region
            block["by_region"][region] = block["by_region"].get(region, 0) + 1
    blocks.append(block)
    body = max([b["vector"] for b in blocks if b["region"] == "walk"] or [0])
    res = {"kernel": name, "regions": {r: counts[r] for r in order}, "walk_block": body}
    if lanes:
        res["dynamic"] = dynamic_estimate(name, blocks, lanes)
    for l in asm_lines[end:end + 80]:                               # the resource summary behind the function
        m = re.match(r";\s*(NumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", l.strip())
        if m:
            res[m.group(1)] = int(m.group(2))
    return res


PER_BATCH = ("staging", "masks + lists", "write-out")


def dynamic_estimate(name, blocks, lanes):
    """{region: {"blocks", "static", "trips", "vector_M"}} for the per-batch regions (see the module docstring)."""
    side = lanes["bwd" if "k_render_bwd" in name else "fwd"]
    staging_waves = lanes["pairs"] / 64.0 + side["nonempty_tiles"] / 2.0
    out = {}
    for r in PER_BATCH:
        base = side["wave_batches"] if r == "masks + lists" else staging_waves
        n = static = dyn = 0
        for b in blocks:
            v = b["by_region"].get(r, 0)
            if v:
                n += 1
                static += v
                dyn += v * base * (4 if b["loops"] and r == "write-out" else 1)
        if n:
            out[r] = {"blocks": n, "static": static, "trips": int(round(base)), "vector_M": round(dyn / 1e6, 2)}
    return out


def show_dynamic(res, before=None):
    print("| region (per staged batch) | blocks | static vector | trips per launch | dynamic vector, M per launch |")
    print("|---|---|---|---|---|")
    tot = totb = 0.0
    zero = {"blocks": 0, "static": 0, "trips": 0, "vector_M": 0.0}
    for r in PER_BATCH:
        a, b = res["dynamic"].get(r), ((before or {}).get("dynamic") or {}).get(r)
        if a is None and b is None:
            continue
        a, b = a or zero, b or a or zero
        cell = lambda k, f="%s": (f % a[k]) if a[k] == b[k] else (f + " -> " + f) % (b[k], a[k])
        tot += a["vector_M"]; totb += b["vector_M"]
        print("| " + r + " | " + cell("blocks") + " | " + cell("static") + " | " + cell("trips") + " | " + cell("vector_M", "%.2f") + " |")
    print("| **per-batch regions** | | | | " + ("%.2f" % tot if tot == totb else "%.2f -> %.2f (%+.2f)" % (totb, tot, tot - totb)) + " |")
    print()


def show(res, before=None):
    print("#### `%s`" % res["kernel"])
    head = ["region"] + list(CLASSES)
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    regs = list(res["regions"])
    if before:
        regs += [r for r in before["regions"] if r not in res["regions"]]
    tot = dict.fromkeys(CLASSES, 0)
    totb = dict.fromkeys(CLASSES, 0)
    zero = dict.fromkeys(CLASSES, 0)
    def cell(b, a):
        return "%d" % a if before is None else ("%d" % a if a == b else "%d -> %d" % (b, a))
    for r in regs:
        a, b = res["regions"].get(r, zero), (before["regions"].get(r, zero) if before else zero)
        for c in CLASSES:
            tot[c] += a[c]; totb[c] += b[c]
        print("| " + r + " | " + " | ".join(cell(b[c], a[c]) for c in CLASSES) + " |")
    print("| **total** | " + " | ".join(cell(totb[c], tot[c]) for c in CLASSES) + " |")
    extra = ["walk_block", "NumVgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
    print()
    print(", ".join("%s %s" % (k, (("%s -> %s" % (before.get(k), res[k])) if before and before.get(k) != res.get(k) else res[k]))
                    for k in extra if k in res))
    print()
    if "dynamic" in res:
        show_dynamic(res, before)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernels", nargs="+", help="substrings of the mangled kernel names")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="source tree to compile (default: this one)")
    ap.add_argument("--keep-asm", dest="keep_asm", help="keep the compiled assembly here (for --asm)")
    ap.add_argument("--asm", help="use this assembly file (made with -gline-tables-only) instead of compiling")
    ap.add_argument("--dump", metavar="REGION", help="also list the instructions of this region (with every block label)")
    ap.add_argument("--json", help="write the counts here")
    ap.add_argument("--before", help="counts of an earlier tree (--json): print before -> after")
    ap.add_argument("--dynamic", metavar="LANES.jsonl", help="also estimate the per-batch regions' dynamic vector count from this counted launch")
    ap.add_argument("--config", default="C2", help="--dynamic: the record's config (default C2)")
    ap.add_argument("--opacity", default="A", help="--dynamic: the record's opacity scenario (default A)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if a.asm:
        lines = open(a.asm).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "t4d_raster.s")
            cwd = os.getcwd()
            os.chdir(root)                                           # relative paths in the line tables resolve against the tree
            try:
                compile_asm(root, out)
            finally:
                os.chdir(cwd)
            lines = open(out).read().split("\n")
            if a.keep_asm:
                open(a.keep_asm, "w").write("\n".join(lines))
    lanes = None
    if a.dynamic:
        recs = [json.loads(l) for l in open(a.dynamic) if l.strip()]
        lanes = next(r for r in recs if r["config"] == a.config and r["opacity"] == a.opacity)
    results = [census(lines, k, root, a.dump, lanes) for k in a.kernels]
    before = {r["kernel"]: r for r in json.load(open(a.before))} if a.before else {}
    for r in results:
        show(r, before.get(r["kernel"]))
    if a.json:
        json.dump(results, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
