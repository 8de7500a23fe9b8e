"""Timeline of the critical wave of k_sba_lm's row instance on the benchmark problem, from the
diagnostic library of tools/probe/lm_timeline_probe.hip (build line there):

    ACINOSET_HIP_LIB=tools/probe/libacinoset_lm_timeline.so python tools/lm_timeline.py [tag] [out.txt]

WARM launches back to back on one stream, then MEAS more without a gap, each writing its waves'
stamps (7 x s_memtime, 1 x s_memrealtime span) to a slice of its own. Ticks become ns through the
clock each wave measured itself: (last - first s_memtime) / s_memrealtime span x 100 MHz, median
over all waves and launches. Printed per segment: the median over the measured launches for the
wave that holds point 251 (the headline's slowest point, wave 251 // 4), and the median over all
waves.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from acinoset_amd import _native, workloads

WARM, MEAS, POINT = 56, 16, 251
SEGMENTS = ('entry -> first vector wait over', 'first -> last vector wait over', 'last vector wait -> loop entry',
            'loop (entry -> exit)', 'loop exit -> before the store\'s wait', 'the wait ahead of the final store',
            'whole wave (entry -> store)')


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else 'tree'
    ctx = _native.Context(0)
    if not hasattr(ctx.lib, 'acs_sba_lm_stamps'):
        sys.exit('the loaded library has no acs_sba_lm_stamps: set ACINOSET_HIP_LIB to the diagnostic build')
    ctx.lib.acs_sba_lm_stamps.argtypes = [C.c_void_p]
    dev = torch.device('cuda', 0)
    wl = workloads.sba_reference_workload()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cams, d_uv, d_mask, d_pts0 = T(wl.cams), T(wl.uv), T(wl.mask), T(wl.pts0)
    d_pts = d_pts0.clone()
    n_pts, n_cams = wl.mask.shape
    assert ctx.sba_lm_layout(n_cams, n_pts)[0] == 'row'
    n_waves = (n_pts * 16 + 63) // 64
    buf = torch.zeros((MEAS + 1, n_waves, 8), dtype=torch.int64, device=dev)
    opts = _native.Context.sba_opts()
    torch.cuda.synchronize()
    for i in range(WARM + MEAS):
        k = 0 if i < WARM else i - WARM + 1          # the warm launches share slice 0
        ctx.lib.acs_sba_lm_stamps(C.c_void_p(buf[k].data_ptr()))
        ctx.sba_points_dense_dev(d_cams.data_ptr(), n_cams, d_uv.data_ptr(), d_mask.data_ptr(), n_pts, d_pts.data_ptr(),
                                 opts, pts_in_p=d_pts0.data_ptr())
    ctx.sync()
    ctx.lib.acs_sba_lm_stamps(None)
    s = buf[1:].cpu().numpy().astype(np.float64)   # (MEAS, n_waves, 8)
    ticks, rt = s[..., 6] - s[..., 0], s[..., 7]
    ghz = float(np.median(ticks / rt)) * 0.1        # ticks per 10 ns
    seg = np.concatenate([np.diff(s[..., :7], axis=-1), ticks[..., None]], axis=-1) / ghz   # ns
    crit = POINT // 4
    slowest = int(np.argmax(np.median(ticks, axis=0)))
    lines = ['%s: %d waves, %d launches after %d warm ones, s_memtime at %.3f GHz; slowest wave %d (point 251 is in %d)' % (
        tag, n_waves, MEAS, WARM, ghz, slowest, crit),
        '%-40s %12s %12s' % ('segment, ns', 'wave %d' % crit, 'all waves')]
    for i, name in enumerate(SEGMENTS):
        lines.append('%-40s %12.1f %12.1f' % (name, np.median(seg[:, crit, i]), np.median(seg[..., i])))
    text = '\n'.join(lines)
    print(text, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
