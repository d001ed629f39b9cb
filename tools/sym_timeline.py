#!/usr/bin/env python3
"""Per-workgroup timeline of sym_gemv_kernel (diagnostic build: tools/build_variant.sh NAME -DSYM_TIMELINE, loaded through CONP_LIB).
Prints, for the last update, when the workgroups end, how many share a CU, and whether the CUs that stream three tiles set the end
of the launch (528 tiles on 256 CUs at the headline size: sixteen CUs hold three)."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from conp_amd import FixConp, neighbor

wl = sys.argv[1] if len(sys.argv) > 1 else "headline"
s = bench.make_workload(wl)
at, alist, blist = neighbor.build_lists(s)
fx = FixConp(s, device=0)
fx.init_lists(alist, blist); fx.setup_post_neighbor(at); fx.linalg_setup(at)
d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda(); d_q = torch.from_numpy(at.q.copy()).cuda()
lib = ctypes.CDLL(os.environ["CONP_LIB"])
ne_pad = (fx.info().elenum_all + 127) // 128 * 128
nb = ne_pad // 128
ntile = nb * (nb + 1) // 2
buf = (ctypes.c_ulonglong * (3 * ntile))()
for rep in range(44):
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    if rep < 40:
        continue
    torch.cuda.synchronize()
    rc = lib.conp_debug_sym_timeline(buf, ntile)
    a = np.frombuffer(buf, dtype=np.uint64).reshape(ntile, 3).copy()
    t = (a[:, :2].astype(np.int64) - a[:, 0].astype(np.int64).min()) * 0.01      # us
    hw = a[:, 2] & 0xffffffff; xcc = (a[:, 2] >> 32).astype(np.int64)
    cu = (hw >> 8) & 0xf; sh = (hw >> 12) & 0x1; se = (hw >> 13) & 0x7
    key = (xcc << 16) | (se.astype(np.int64) << 8) | (sh.astype(np.int64) << 4) | cu.astype(np.int64)
    u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    per_cu = cnt[inv]                                   # tiles on this workgroup's CU
    end = t[:, 1]
    med = np.median(end)
    order = np.argsort(end)[::-1]
    print(f"update {rep}: rc {rc}, {ntile} workgroups on {len(u)} CUs, tiles per CU: " +
          ", ".join(f"{k}: {int((cnt == k).sum())} CUs" for k in sorted(set(cnt.tolist()))))
    print("  start min/median/max %.2f %.2f %.2f us; end percentiles 10/50/90/99/100: %.2f %.2f %.2f %.2f %.2f" %
          ((t[:, 0].min(), np.median(t[:, 0]), t[:, 0].max()) + tuple(np.percentile(end, [10, 50, 90, 99, 100]))))
    print("  lifetime median %.2f max %.2f us" % (np.median(end - t[:, 0]), (end - t[:, 0]).max()))
    for k in sorted(set(cnt.tolist())):
        m = per_cu == k
        print("  workgroups on CUs with %d tiles: %4d, end median %.2f max %.2f us, lifetime median %.2f" %
              (k, int(m.sum()), np.median(end[m]), end[m].max(), np.median((end - t[:, 0])[m])))
    last = order[:16]
    print("  the 16 last workgroups end %.2f .. %.2f us (%.2f .. %.2f behind the median); tiles on their CUs: %s; diagonal tiles among them: %d" %
          (end[last].min(), end[last].max(), end[last].min() - med, end[last].max() - med, per_cu[last].tolist(),
           sum(1 for b in last if any(b == i * (i + 1) // 2 + i for i in range(nb)))))
    xe = [end[xcc == x].max() for x in range(8) if (xcc == x).any()]
    print("  last end per XCD:", " ".join("%.2f" % v for v in xe))
