"""Stand-alone timing of sf_local_scan_banded_batch (the score scan for new local kernels on the band + Woodbury solver).
    python tools/bench_local_scan_banded.py N B [runs]
One synthetic order of N pixels (m = 4), B walkers of the model with a global and one local kernel, every pixel x the widths 8, 15
and 30 km/s as candidates (3 N of them).  Between device events, every call synchronised, `runs` runs (default 5) of one timed
call each behind one untimed call, median and range in ms per call:
  sf_local_scan_banded_batch                     the whole call
  sf_local_scan_batch                            the same scan on the dense factor
  sf_diagnose_banded_batch, want_cinv_diag       the banded call's head (own residual) at the scan's half-width, with the read-out of
                                                 diag(C^-1), and the same at the walkers' own half-width bound
  sf_loglike_banded_batch                        the likelihood at the walkers' own half-width bound
and the largest banded-against-dense difference per number over the dense number's size (|dense|, and the largest |dense| of the
scan).  Counts printed beside them: the bytes of the tiles of W that the banded call writes and its candidates read."""
import statistics
import sys

import numpy as np
import torch
from _bench_common import order_and_walkers, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

N, B = int(sys.argv[1]), int(sys.argv[2])
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
lib = _lib.require_gpu()
SIGMAS = (8.0, 15.0, 30.0)


def spread(call):
    ms = [timed(call, 1) for _ in range(runs)]
    return f"{statistics.median(ms):9.3f} ms (range {min(ms):.3f} .. {max(ms):.3f}, {runs} runs)"


o, do, walkers = order_and_walkers(N, B)
md, rows = pack_rows(do, walkers)
dev = do.dev
cand = np.array([(w, s) for s in SIGMAS for w in o["wave"]])
ncand = len(cand)
hw = do.halfwidth_bound(md, rows)
wmax = do.local_scan_banded_max_patch(md) - 1
W = int(hw.max())
lo, hi = D.local_scan_patches(o["wave"], cand)
assert W <= wmax and (hi - lo + 1).max() <= wmax + 1, (W, wmax, int((hi - lo + 1).max()))
nbr = -(-N // 64)
tiles = 8 * B * nbr * (2 * min(nbr - 1, 3) + 1) * 4096
with torch.cuda.device(dev):
    P, Cd = D.to_dev(rows, dev), D.to_dev(cand, dev)
    lnl, lnl_d, lnl_l = D.empty((B,), dev), D.empty((B,), dev), D.empty((B,), dev)
    out, out_d = D.empty((B, ncand, 3), dev), D.empty((B, ncand, 3), dev)
    alpha, cinv_diag = D.empty((B, 1, N), dev), D.empty((B, N), dev)
    info, info_d = D.empty((B,), dev, torch.int32), D.empty((B,), dev, torch.int32)
    ws = do._reserve(max(do.local_scan_banded_workspace_bytes(md, B, ncand), do.local_scan_workspace_bytes(md, B, ncand),
                         do.diagnose_banded_workspace_bytes(md, B, wmax, 1, True, False), do.banded_workspace_bytes(md, B, W)))
    t_like = spread(lambda: do._call("loglike_banded_batch", md, B, P, W, lnl_l, None, None, None, None, info, ws=ws))
    t_head = {w: spread(lambda: do._call("diagnose_banded_batch", md, B, P, w, None, 1, N, 0, alpha, cinv_diag, None, None, None, info,
                                         ws=ws)) for w in (wmax, W)}
    t_band = spread(lambda: do._call("local_scan_banded_batch", md, B, P, Cd, ncand, out, lnl, info, ws=ws))
    t_dense = spread(lambda: do._call("local_scan_batch", md, B, P, Cd, ncand, out_d, lnl_d, info_d, ws=ws))
    assert int(info.abs().max()) == 0 and int(info_d.abs().max()) == 0 and bool(torch.isfinite(out).all())
    got, ref = out.cpu().numpy(), out_d.cpu().numpy()
print(f"N={N} B={B} m=4, {ncand} candidates, half-width of the scan {wmax}, of the walkers {W}; tiles of W: {tiles / 1e9:.3f} GB written "
      f"once")
print(f"  sf_local_scan_banded_batch                     {t_band}")
print(f"  sf_local_scan_batch (dense)                    {t_dense}")
print(f"  sf_diagnose_banded_batch cinv_diag, W = {wmax:3d}    {t_head[wmax]}")
print(f"  sf_diagnose_banded_batch cinv_diag, W = {W:3d}    {t_head[W]}")
print(f"  sf_loglike_banded_batch, W = {W:3d}               {t_like}")
for i, key in enumerate(("quad", "trace", "fisher")):
    d = np.abs(got[..., i] - ref[..., i])
    size = np.abs(ref[..., i])
    print(f"  {key:6s}: largest |banded - dense| / |dense| {np.max(d[size > 0] / size[size > 0]):.3g}, / largest |dense| {d.max() / size.max():.3g}")
print(f"  lnl: largest |banded - dense| / |dense| {float(((lnl - lnl_d).abs() / lnl_d.abs()).max()):.3g}", flush=True)
