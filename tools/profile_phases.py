#!/usr/bin/env python3
"""Per-phase cycle breakdown of the wave pipeline from a QHUFF_PROFILE build
(make -C ls-qpack_amd prof; run with QHUFF_LIB=.../libqhuff_prof.so).
Slots per wave iteration (qhuff_pipeline.h): 0 top, 1 after the top wait,
2 after stage + loads + polls, 3 after codec + scan, 9 after lb.start +
emit, 4 after the poll wait, 7 after the older tile's look-back (inside the
flush), 5 after the flush, 6 end of iteration (after the gather); 10 (inside the poll wait) once all
but lb.start's two operations have landed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-qpack_amd"))
os.environ.setdefault("QHUFF_LIB", os.path.join(ROOT, "ls-qpack_amd",
                                                "libqhuff_prof.so"))

import numpy as np
import torch
import qhuff

ITERS, SLOTS = 16, 12
NAMES = ["top wait", "stage+loads+polls", "codec+scan", "start+emit+wait",
         "flush", "gather"]


def report(tag, p):
    p = p.reshape(-1, ITERS, SLOTS).astype(np.int64)
    live = p[:, :, 0] != 0
    waves = int(live[:, 0].sum())
    t0 = p[live[:, 0], 0, 0].min()
    print("%s: %d waves, iterations/wave %.2f" % (tag, waves,
                                                  live.sum() / max(waves, 1)))
    for ph in range(6):
        a, b = p[:, :, ph], p[:, :, ph + 1]
        ok = live & (a != 0) & (b != 0)
        d = (b - a)[ok]
        if d.size:
            print("  %-12s mean %8.0f  p50 %8.0f  p90 %8.0f  max %8.0f cyc"
                  % (NAMES[ph], d.mean(), np.median(d), np.percentile(d, 90),
                     d.max()))
    # shader clock: s_memtime cycles over s_memrealtime (100 MHz) ticks
    # between a wave's first and last iteration starts
    nit = live.sum(axis=1)
    sel = nit >= 2
    if sel.any():
        rows = np.nonzero(sel)[0]
        last = nit[sel] - 1
        dm = p[rows, last, 0] - p[rows, 0, 0]
        dr = p[rows, last, 11] - p[rows, 0, 11]
        good = dr > 0
        if good.any():
            mhz = 100.0 * dm[good] / dr[good]
            print("  shader clock  p10 %.0f  p50 %.0f  p90 %.0f MHz (s_memtime / s_memrealtime)"
                  % (np.percentile(mhz, 10), np.median(mhz), np.percentile(mhz, 90)))
    # (decode builds) wave entry and after-barrier wall clock, iteration 15
    pe, pb_ = p[:, ITERS - 1, 10], p[:, ITERS - 1, 11]
    sel2 = live[:, 0] & (pe > 0) & (pb_ > 0)
    if sel2.any():
        base = pe[sel2].min()
        ent = (pe[sel2] - base) * 0.01
        pro = (pb_[sel2] - pe[sel2]) * 0.01
        fst = (p[sel2, 0, 11] - pb_[sel2]) * 0.01
        print("  wave entry (us after the first): p50 %.2f max %.2f | prologue to barrier p50 %.2f max %.2f | barrier to first iteration p50 %.2f max %.2f"
              % (np.median(ent), ent.max(), np.median(pro), pro.max(), np.median(fst), fst.max()))
    # wall-clock (100 MHz) of each wave's first iteration start and last
    # iteration start, relative to the earliest wave: dispatch skew and span
    r0 = p[live[:, 0], 0, 11]
    if (r0 > 0).all() and len(r0):
        base = r0.min()
        st = (r0 - base) * 0.01
        lastr = np.array([p[i, live[i].sum() - 1, 11] for i in np.nonzero(live[:, 0])[0]])
        en = (lastr - base) * 0.01
        print("  wave first-iteration start (us after the earliest): p50 %.2f  p90 %.2f  max %.2f;"
              "  last-iteration start max %.2f us" % (np.median(st), np.percentile(st, 90), st.max(), en.max()))
    ok = live & (p[:, :, 4] != 0) & (p[:, :, 7] != 0)
    if ok.any():
        lbt = (p[:, :, 7] - p[:, :, 4])[ok]
        stt = (p[:, :, 5] - p[:, :, 7])[ok]
        raw = p[:, :, 8][ok]
        w1, w2, w3 = raw & 0xfff, (raw >> 12) & 0xfff, raw >> 24
        sp = w1 + w2                            # re-polls of either window
        print("  flush: look-back mean %.0f p90 %.0f | stores mean %.0f | re-polls mean %.2f, >0 in %.1f%%, max %d"
              % (lbt.mean(), np.percentile(lbt, 90), stt.mean(), sp.mean(),
                 100.0 * (sp > 0).mean(), sp.max()))
        print("  re-polls: tile window mean %.2f (>0 in %.1f%%) | super windows mean %.2f (>0 in %.1f%%) | windows past two mean %.2f (>0 in %.1f%%)"
              % (w1.mean(), 100.0 * (w1 > 0).mean(), w2.mean(),
                 100.0 * (w2 > 0).mean(), w3.mean(), 100.0 * (w3 > 0).mean()))
    # (iteration 14 belongs to the drain: slots 6-8 its stamps, slots 9-11
    # the re-poll counts of its look-backs with the tile in the upper half,
    # qhuff_pipeline.h -- no timestamps, so it stays out of the means below)
    live = live.copy()
    live[:, ITERS - 2] = False
    ok = live & (p[:, :, 3] != 0) & (p[:, :, 9] != 0) & (p[:, :, 4] != 0)
    if ok.any():
        a = (p[:, :, 9] - p[:, :, 3])[ok]
        b = (p[:, :, 4] - p[:, :, 9])[ok]
        print("  start+emit mean %.0f p90 %.0f | poll wait mean %.0f p90 %.0f"
              % (a.mean(), np.percentile(a, 90), b.mean(), np.percentile(b, 90)))
    ok = live & (p[:, :, 9] != 0) & (p[:, :, 10] != 0) & (p[:, :, 4] != 0)
    if ok.any():
        a = (p[:, :, 10] - p[:, :, 9])[ok]
        b = (p[:, :, 4] - p[:, :, 10])[ok]
        print("  poll wait split: older ops mean %.0f p90 %.0f | own start "
              "(aggregate store + super add) mean %.0f p90 %.0f"
              % (a.mean(), np.percentile(a, 90), b.mean(), np.percentile(b, 90)))
    if os.environ.get("SLOW"):
        slow_report(p, live)
    if not os.environ.get("TIMELINE"):
        return
    # timeline: start of iterations relative to the first stamp (s_memtime
    # counters; waves on different XCDs may be skewed)
    for it in range(0, ITERS):
        ok = live[:, it]
        if not ok.any():
            break
        # relative to each wave's own first stamp (counters of different
        # XCDs are not synchronised)
        s = p[ok, it, 0] - p[ok, 0, 0]
        e = p[ok, it, 6] - p[ok, 0, 0]
        e = e[p[ok, it, 6] != 0]
        print("  iter %2d: waves %5d  start p50 %8.0f max %8.0f   end p50 %8.0f max %8.0f"
              % (it, ok.sum(), np.median(s), s.max(),
                 np.median(e) if e.size else 0, e.max() if e.size else 0))
        # this iteration's phases (mean cycles), same order as above
        ph = []
        for k in range(6):
            a, b = p[ok, it, k], p[ok, it, k + 1]
            g = (a != 0) & (b != 0)
            ph.append((b - a)[g].mean() if g.any() else 0.0)
        print("           phases " + " ".join("%6.0f" % x for x in ph))


def slow_report(p, live):
    """Which waves are slow: wall time (s_memrealtime, 10 ns) per iteration
    over iterations 0..3 of each wave, grouped by XCD (block % 8), by the
    wave's index in its workgroup and by its age rank on its SIMD (w >> 2)."""
    W = 12
    ok = live[:, 4]
    rows = np.nonzero(ok)[0]
    per = (p[rows, 4, 11] - p[rows, 0, 11]) * 10.0 / 4        # ns/iteration
    blk, w = rows // W, rows % W
    print("  per-iteration wall time (ns): mean %.0f p10 %.0f p50 %.0f p90 %.0f max %.0f"
          % (per.mean(), np.percentile(per, 10), np.median(per),
             np.percentile(per, 90), per.max()))
    for name, key, n in (("XCD (block % 8)", blk % 8, 8),
                         ("wave in workgroup", w, W),
                         ("age rank on SIMD (w >> 2)", w >> 2, 3)):
        means = [per[key == k].mean() for k in range(n)]
        print("  by %-26s %s" % (name, " ".join("%.0f" % m for m in means)))
    # each wave's end: its last iteration's start (realtime) plus that
    # iteration's length in cycles at the shader clock (~2.2 GHz)
    nit = live.sum(axis=1)
    allw = np.nonzero(live[:, 0])[0]
    last = nit[allw] - 1
    r0 = p[allw, 0, 11].min()
    end_us = ((p[allw, last, 11] - r0) * 0.01
              + (p[allw, last, 6] - p[allw, last, 0]) / 2200.0)
    wa = (allw % W) >> 2
    print("  wave end (us after the first start): p50 %.2f p90 %.2f max %.2f"
          " | by age rank max %s | tiles per wave by age rank %s"
          % (np.median(end_us), np.percentile(end_us, 90), end_us.max(),
             " ".join("%.2f" % end_us[wa == k].max() for k in range(3)),
             " ".join("%.2f" % nit[allw][wa == k].mean() for k in range(3))))
    cu = np.array([per[blk == b].mean() for b in np.unique(blk)])
    print("  by CU (block): mean %.0f sd %.0f min %.0f max %.0f | within-CU sd "
          "%.0f" % (cu.mean(), cu.std(), cu.min(), cu.max(),
                    np.mean([per[blk == b].std() for b in np.unique(blk)])))


def main():
    n = int(os.environ.get("N", 1 << 20))
    wl = os.environ.get("WORKLOAD", "synthetic")
    if wl == "corpus":
        from qhuff import workload
        data, off = workload.corpus_batch(
            n, os.path.join(ROOT, "tests", "golden", "data"))
    else:
        data, off = qhuff.synth_batch(n)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(off.view(np.int32)).to(dev)
    codec = qhuff.Codec(0)
    # each launch waited for: the variant history (qhuff_host.cpp pick_full)
    # then runs the full kernel from the second launch on, as in a steady
    # stream -- three launches issued back to back all run the first choice
    for _ in range(3):
        h, ho = codec.encode(d, o, 0)
        torch.cuda.synchronize()
    pe = codec.profile_read()
    report("encode", pe)
    hb = int(ho[-1].item())
    h = h[:hb].clone()
    for _ in range(3):
        codec.decode(h, ho)
        torch.cuda.synchronize()
    pd = codec.profile_read()
    report("decode", pd)
    if os.environ.get("RAW"):
        # raw stamps for offline analysis (tools/tail_report.py)
        np.savez_compressed(os.environ["RAW"], encode=pe, decode=pd)
    codec.close()


if __name__ == "__main__":
    main()
