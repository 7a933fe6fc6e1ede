"""What the GPU tests of the stereo stages share: the device handle, a context per case configuration, and the route that puts
constructed tables in front of k_stereo_points, k_stereo_median and k_stereo_lines.

The three kernels read their tables from the result record, so constructed tables need no entry point of their own (the route is
described next to Frontend.batch_run_device): run the whole front-end on the case's images, overwrite counts / keypoints /
descriptors / keylines / line descriptors of the record on the device, run the two stereo stages alone, read uright, depth, disp, le,
counts[4], counts[5] and, through DBG_STEREO_SAD, the SADs and best indices.

Every table passes helpers_matchers.validate_tables with the context's capacities before it goes to the device.
"""
import numpy as np
import pytest

import helpers_matchers as hm


def device():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend

    class G:
        pass
    g = G()
    g.capi, g.Frontend, g.torch = capi, Frontend, torch
    return g


def group_key(c):
    return bytes(c["cfg"])


def run_batch(g, fe, cases):
    """cases: one per frame of the batch.  -> per frame (record dict, sad, best_idx)."""
    torch, capi = g.torch, g.capi
    Y = fe.layout
    F = len(cases)
    W, H = fe.cfg.width, fe.cfg.height
    imgs = np.full((F, 2, H, W), 100, np.uint8)
    for f, c in enumerate(cases):
        hm.validate_tables(c, kp_cap=fe.kp_cap, kl_cap=fe.kl_cap)
        assert (c["W"], c["H"], c["nlevels"]) == (W, H, fe.cfg.orb_nlevels)
        if c["L"] is not None:
            imgs[f, 0], imgs[f, 1] = c["L"], c["R"]
    dimg = torch.from_numpy(imgs).cuda()
    dtab = torch.zeros(fe.table_bytes(F), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (F, dimg.data_ptr(), dimg.data_ptr() + W * H, W, 2 * W * H, dtab.data_ptr())
    fe.batch_run_device(*args, stages=capi.RUN_ALL)
    fe.sync()
    tab = dtab.cpu().numpy().copy()
    for f, c in enumerate(cases):
        rec = tab[f * Y.record_bytes:(f + 1) * Y.record_bytes]
        counts = rec[Y.off_counts:Y.off_counts + 32].view(np.int32)
        counts[0], counts[1], counts[2], counts[3] = len(c["kpL"]), len(c["kpR"]), len(c["klL"]), len(c["klR"])
        counts[4] = counts[5] = -7                      # (must be rewritten by the stereo stages)
        for e, k in enumerate("LR"):
            for off, arr in ((Y.off_kp[e], c["kp" + k]), (Y.off_desc[e], c["desc" + k]), (Y.off_kl[e], c["kl" + k]),
                             (Y.off_ldesc[e], c["ld" + k])):
                b = np.ascontiguousarray(arr).view(np.uint8).ravel()
                rec[off:off + b.size] = b
        n, m = len(c["kpL"]), len(c["klL"])
        rec[Y.off_uright:Y.off_uright + 4 * n].view(np.float32)[:] = 123.0
        rec[Y.off_depth:Y.off_depth + 4 * n].view(np.float32)[:] = 123.0
        rec[Y.off_disp:Y.off_disp + 8 * m].view(np.float32)[:] = 123.0
        rec[Y.off_le:Y.off_le + 24 * m].view(np.float64)[:] = 123.0
    dtab.copy_(torch.from_numpy(tab))
    torch.cuda.synchronize()
    fe.batch_run_device(*args, stages=capi.RUN_STEREO_POINTS | capi.RUN_STEREO_LINES)
    fe.sync()
    tab = dtab.cpu().numpy()
    out = []
    for f in range(F):
        raw = fe.debug_fetch(2 * f, capi.DBG_STEREO_SAD).view(np.int32)
        out.append((fe.parse_record(tab, f), raw[:fe.kp_cap].copy(), raw[fe.kp_cap:2 * fe.kp_cap].copy()))
    return out


def make_frontend(g, c, max_frames, lsd_nfeatures, orb_nfeatures=2000):
    cfg = g.capi.Config.from_buffer_copy(bytes(c["cfg"]))
    cfg.max_frames, cfg.orb_nfeatures, cfg.lsd_nfeatures = max_frames, orb_nfeatures, lsd_nfeatures
    fe = g.Frontend(cfg)
    fe.debug_enable(True)
    return fe
