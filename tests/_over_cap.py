"""Helper of the tests/_*_device_path.py scripts: a frame pass on device memory while the handle already holds more than
option max_device_mb allows.  The frame is 192 x 96: the denoisers' scratch for it, 64 bytes per texel, is 1.125 MiB, which
a cap of 1 MiB cannot hold, and no call on device memory allocates anything else."""
import numpy as np
import torch

import ray_tracer_2_amd as rt

W, H = 192, 96
CHANNELS = ("dir", "point", "normal", "object", "albedo", "emission")


def frame(t, seed=0):
    """The G-buffer of a W x H frame, on the host and on the device, and an (H, W, 4) colour plane of positive noise."""
    p = rt.make_params(W, H, 1, 1)
    color = np.random.default_rng(seed).random((H, W, 4), np.float32) + np.float32(0.25)
    return t.render_gbuffer(p, CHANNELS), t.render_gbuffer(p, CHANNELS, device=True), color


def hold_denoise_scratch(t, dev_g, color):
    """One good rt_denoise on the frame: the handle then holds the 1.125 MiB scratch."""
    t.denoise({k: dev_g[k] for k in ("normal", "point")}, color, 1)
    t.synchronize()
    assert t.last_launch()["device_mb_held"] >= 2


def _bytes(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def over_cap(t, call, outs, wants, refused, what):
    """call() -- a device-memory call that has run before and writes the tensors `outs` -- under a cap of 1 MiB that the
    handle already exceeds: refused with RT_ERR_OUT_OF_MEMORY and the outputs untouched (`refused`), or done with the bits
    `wants`; then once more without the cap, which gives those bits either way."""
    assert t.last_launch()["device_mb_held"] >= 2, what
    held = t.last_launch()["device_mb_held"]
    for o in outs:
        o.view(torch.uint8).fill_(0xA5)
    torch.cuda.synchronize()
    t.set_option("max_device_mb", 1)
    try:
        call()
        was_refused = False
    except rt.RtError as e:
        assert e.code == -8 and "max_device_mb" in str(e), (what, e)
        was_refused = True
    t.synchronize()
    print(what, "over the cap:", "refused" if was_refused else "done", flush=True)
    assert was_refused == refused, what
    assert t.last_launch()["device_mb_held"] == held, what
    for o, w in zip(outs, wants):
        if refused:
            assert (_bytes(o) == 0xA5).all(), (what, "a refused call wrote an output")
        else:
            assert np.array_equal(_bytes(o), _bytes(w)), (what, "over the cap")
    t.set_option("max_device_mb", 0)
    call()
    t.synchronize()
    for o, w in zip(outs, wants):
        assert np.array_equal(_bytes(o), _bytes(w)), (what, "without a cap")
