"""Binning kernels of one default bench run from rocprofv3 output: time per frame (kernel trace) and bytes per frame (PMC runs of
their own) against the byte model of DESIGN.md §3 (round 4).

  python3 profiles/binning_bytes.py --trace DIR --pmc DIR [DIR ...] --pairs P --tris N [--old]

--trace: a `rocprofv3 --kernel-trace` output directory; --pmc: one directory per `rocprofv3 --pmc` run (FETCH_SIZE, WRITE_SIZE,
SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE, ...).  Bytes read = 2 x FETCH_SIZE x 1024 (gfx950 counts half of a wide coalesced read,
MI355X_MICROARCH), bytes written = WRITE_SIZE x 1024, as profiles/summarize_rocprof.py reads them.  --old: the model of the
three-stream layout before round 4 (16-bit keys, k_bounds).
"""
import argparse
import csv
import glob
import re
from collections import defaultdict

BIN = ("k_chunk_spine", "k_expand", "k_radix_hist", "k_radix_scan_rows", "k_radix_scatter", "k_bounds", "k_make_items")


def short(name):
    m = re.search(r"k_radix_scatter<(?:\d+, )?(true|false), (true|false)>", name)
    if m:
        return "k_radix_scatter" + (" (last pass)" if m.group(2) == "true" else "")
    for k in BIN + ("k_setup", "k_raster", "k_fold_stats"):
        if k in name:
            return k
    return name.split("(")[0][:38]


ap = argparse.ArgumentParser()
ap.add_argument("--trace")
ap.add_argument("--pmc", nargs="*", default=[])
ap.add_argument("--pairs", type=int, required=True)
ap.add_argument("--tris", type=int, required=True)
ap.add_argument("--old", action="store_true")
a = ap.parse_args()
P, N = a.pairs, a.tris


def binning(name):
    return name.split(" ")[0] in BIN


if a.trace:
    acc = defaultdict(list)
    for f in glob.glob(f"{a.trace}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            acc[short(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    frames = len(acc["k_setup"])
    print(f"== kernel trace: {frames} frames ==")
    tot = 0.0
    for n, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
        tot += sum(v) / frames if binning(n) else 0.0
        print(f"  {n:38s} calls {len(v):4d}  avg {sum(v) / len(v):8.1f} us  median {sorted(v)[len(v) // 2]:8.1f} us  per frame {sum(v) / frames:8.1f} us")
    print(f"  binning kernels per frame: {tot:.1f} us\n")

if a.pmc:
    # per kernel, per counter: the mean over dispatches of the sum over the dispatch's rows
    cnt = defaultdict(lambda: defaultdict(list))
    for d in a.pmc:
        for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
            per = defaultdict(float)
            for r in csv.DictReader(open(f)):
                n = short(r["Kernel_Name"])
                if binning(n):
                    per[(n, r["Dispatch_Id"], r["Counter_Name"])] += float(r["Counter_Value"])
            for (n, disp, c), v in per.items():
                cnt[n][c].append(v)
    # passes per frame of each kernel name (two radix passes at <= 65536 tiles; one of them the last pass from round 4 on)
    per_frame = {"k_radix_hist": 2, "k_radix_scan_rows": 2, "k_radix_scatter": 2 if a.old else 1}
    # byte model per dispatch: reads, writes
    if a.old:
        model = {"k_expand": (12 * N, 8 * P), "k_radix_hist": (2 * P, 0), "k_radix_scatter": (8 * P, 8 * P), "k_bounds": (2 * P, 0)}
    else:
        model = {"k_expand": (12 * N, 8 * P), "k_radix_hist": (4 * P, 0), "k_radix_scatter": (8 * P, 8 * P),
                 "k_radix_scatter (last pass)": (8 * P, 6 * P)}
    print("== PMC per dispatch (means) ==")
    for n in sorted(cnt):
        cs = cnt[n]
        print(f"  {n:30s} " + "  ".join(f"{c}={sum(v) / len(v):.4g}" for c, v in sorted(cs.items())))
        act, conf = sum(cs.get("SQ_LDS_IDX_ACTIVE", [0])), sum(cs.get("SQ_LDS_BANK_CONFLICT", [0]))
        if act:
            print(f"  {'':30s} SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = {conf / act:.3f}")
    print(f"\n== bytes per frame (P = {P} pairs, N = {N} triangles; MB = 1e6 B) ==")
    print(f"  {'kernel':30s} {'x':>2s} {'read':>8s} {'model':>8s} {'write':>8s} {'model':>8s}")
    tr = tw = mr = mw = 0.0
    for n in sorted(cnt):
        cs = cnt[n]
        if "FETCH_SIZE" not in cs or "WRITE_SIZE" not in cs:
            continue
        k = per_frame.get(n, 1)
        r = 2 * 1024 * sum(cs["FETCH_SIZE"]) / len(cs["FETCH_SIZE"]) * k
        w = 1024 * sum(cs["WRITE_SIZE"]) / len(cs["WRITE_SIZE"]) * k
        m_r, m_w = (x * k for x in model.get(n, (0, 0)))
        tr += r; tw += w; mr += m_r; mw += m_w
        print(f"  {n:30s} {k:2d} {r / 1e6:8.1f} {m_r / 1e6:8.1f} {w / 1e6:8.1f} {m_w / 1e6:8.1f}"
              + (f"   read {100 * (r / m_r - 1):+.0f} %" if m_r else "") + (f", write {100 * (w / m_w - 1):+.0f} %" if m_w else ""))
    print(f"  {'total':30s}    {tr / 1e6:8.1f} {mr / 1e6:8.1f} {tw / 1e6:8.1f} {mw / 1e6:8.1f}")
    print(f"  measured {(tr + tw) / 1e6:.1f} MB against the model's {(mr + mw) / 1e6:.1f} MB: {100 * ((tr + tw) / (mr + mw) - 1):+.1f} %")
