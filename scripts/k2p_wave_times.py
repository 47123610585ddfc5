#!/usr/bin/env python3
"""How the two sweeping wavefronts of a SIMD share it in K2p (development helper; needs the timing-only build
`make dbg DBG_FLAGS=-DMI_K2P_DBG_WAVETIMES DBG_NAME=wt` and MI_SA_LIB pointing at it: every sweeping wavefront then
overwrites the first 24 bytes of its replica-A row of states with [HW_ID, XCC_ID, s_memtime before the first sweep,
s_memtime after the last one]; the states of that build are wrong by design).

Runs the bench shape (scripts/perf_k2.py's model, created as bench.py creates it: padded order), groups the records by
(XCC, SE, CU, SIMD) and prints, per SIMD, the sweeping wavefronts' durations, the ratio slowest / quickest and which of
them started first, then the chip-wide distribution of that ratio, the wave-slot pairs and, per XCC, the spread of the
start and of the end ticks (read their difference: the start ticks of one XCC were seen several durations apart).
The model is scripts/perf_k2.py's (that script runs on import, so its few lines are repeated here), and the rows are
read with mi_sa_fetch directly: Problem.fetch() gathers the caller's variables out of their seats.
usage: MI_SA_LIB=.../libmi_sa_wt.so k2p_wave_times.py [--sweeps S] [--replicas R] [--list]"""
import argparse
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrna_seq_qannealing_clustering_amd import _lib, graphs, models  # noqa: E402
from scrna_seq_qannealing_clustering_amd.engine import Problem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=1000)
ap.add_argument("--replicas", type=int, default=4096)
ap.add_argument("--n", type=int, default=2638)
ap.add_argument("--list", action="store_true", help="print every SIMD's line, not only the first sixteen")
a = ap.parse_args()
nodes, eu, ev, w, _ = graphs.synthetic_snn(a.n, 5, 15, 15, 9, seed=0, spread=3.0)
m = models.build_bqm_qubo(graphs.EdgeListGraph(nodes, eu, ev, w), 0.05, k=8)
betas = models.make_beta_schedule(a.sweeps, models.default_beta_range(m))
with Problem.csr_rank1(m.rowptr, m.col, m.val.astype(np.float32), m.lin.astype(np.float32),
                       float(np.float32(m.c_pair)), order="padded", energy_model=(m.val, m.lin, m.c_pair)) as p:
    p.anneal(a.replicas, betas, 1234)          # (clocks and caches warm)
    p.anneal(a.replicas, betas, 1234)
    ms, name = p.kernel_ms(), p.kernel_name()
    # the device's own rows (Problem.fetch gathers the caller's variables out of their seats)
    st = np.empty((a.replicas, p.n_dev), dtype=np.uint8)
    _lib.call("mi_sa_fetch", p._handle(), st, None, np.zeros(3, dtype=np.uint64))
rec = np.ascontiguousarray(st[0::2, :24])
hw = rec[:, 0:4].copy().view(np.uint32)[:, 0]
xcc = rec[:, 4:8].copy().view(np.uint32)[:, 0] & 15
t0 = rec[:, 8:16].copy().view(np.uint64)[:, 0].astype(np.int64)
t1 = rec[:, 16:24].copy().view(np.uint64)[:, 0].astype(np.int64)
slot, simd, cu, se = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 13) & 7
dur = t1 - t0
print("%s: %.3f ms, %d sweeping wavefronts, %d sweeps of %d slots" % (name, ms, len(hw), a.sweeps, p.n_dev // 64))
ok = (dur > 0) & (dur < (1 << 40))
if "pair" not in name or not ok.all():
    for k in range(3):
        print("  row %d: %s" % (2 * k, rec[k].tobytes().hex()))
    sys.exit("%d of %d rows hold no wave-time record: is MI_SA_LIB the -DMI_K2P_DBG_WAVETIMES build?" % ((~ok).sum(), len(ok)))
by = collections.defaultdict(list)
for k in range(len(hw)):
    by[(int(xcc[k]), int(se[k]), int(cu[k]), int(simd[k]))].append(k)
print("SIMDs holding sweeping wavefronts: %d; wavefronts per SIMD: %s" % (
    len(by), dict(collections.Counter(len(v) for v in by.values()))))
print("ticks per slot visit: median %.0f" % np.median(dur / (a.sweeps * (p.n_dev // 64))))
ratios, first_is_quick, slot_pairs = [], 0, collections.Counter()
shown = 0
for key in sorted(by):
    ks = sorted(by[key], key=lambda k: t0[k])                 # by start tick: the first one is the older
    if len(ks) != 2:
        continue
    d = dur[ks]
    ratios.append(d.max() / d.min())
    first_is_quick += int(d[0] <= d[1])
    slot_pairs[(int(slot[ks[0]]), int(slot[ks[1]]))] += 1
    if a.list or shown < 16:
        shown += 1
        print("  xcc %d se %d cu %2d simd %d  slots %d,%d  start +%d  durations %d %d  ratio %.4f  ends %+d" % (
            key + (slot[ks[0]], slot[ks[1]], t0[ks[1]] - t0[ks[0]], d[0], d[1], d.max() / d.min(), t1[ks[1]] - t1[ks[0]])))
r = np.array(ratios)
if len(r):
    print("ratio slowest / quickest of a SIMD's two sweeping wavefronts, %d SIMDs: min %.4f  p10 %.4f  median %.4f  p90 %.4f  "
          "max %.4f  mean %.4f" % ((len(r),) + tuple(np.percentile(r, [0, 10, 50, 90, 100])) + (r.mean(),)))
    print("the wavefront that started first is the quicker one on %d of %d SIMDs" % (first_is_quick, len(r)))
    print("wave-slot pairs (older, younger): %s" % dict(slot_pairs.most_common(12)))
print("durations chip-wide: min %d  median %d  max %d  (max / min %.4f)" % (dur.min(), np.median(dur), dur.max(), dur.max() / dur.min()))
for x in sorted(set(xcc.tolist())):
    s = xcc == x
    e = t1[s]
    print("  xcc %d: %4d wavefronts  end ticks first -> last %d (%.2f %% of the median duration)  start ticks first -> last %d" % (
        x, s.sum(), e.max() - e.min(), 100.0 * (e.max() - e.min()) / np.median(dur[s]), t0[s].max() - t0[s].min()))
