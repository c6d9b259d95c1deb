"""The v2 part-box trainer at its geometry (N 10, T 20, 240x320 frames, S 192, bf16): sfk_roi_resize time, bytes and
fraction of HBM peak; a host-fed v2 training step from uint8 frames + boxes against the same step from the float
pre-resized batch (ms, peak memory); and the host time the loader no longer spends (one clip's F.interpolate on one thread).
--jitter adds sfk_color_jitter (include/sfk_aug.h): its two launches at the v2 and the HTAH (N 55, 21 channels) geometry with
the bytes they must move (three planes read twice and written once) and the effective bandwidth, the same call for clips
without a contrast op (pass 1 exits at once: what is left is pass 2), and the uint8 step with the batch's 'jitter' entry.
Prints one JSON line.  Usage: python tools/bench_v2.py [--steps 10] [--warmup 3] [--jitter]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s


def cuda_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--t", type=int, default=20)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--jitter", action="store_true")
    args = ap.parse_args()
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.config import get_cfg
    from video_classification_amd.input_pipeline import byte_lut
    n, t, h, w, c, s = args.n, args.t, 240, 320, 7, args.size
    dev = "cuda"
    res = {"geometry": f"N{n} T{t} {h}x{w}x{c} -> {s}^2"}
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (n, t, h, w, c), generator=g, dtype=torch.uint8)
    full = torch.tensor([[0, 0, w, h]] * n, dtype=torch.int32)

    # 1. the kernel alone, full-frame boxes (every byte of the frames is read)
    be, lut = HipBackend(), byte_lut().to(dev)
    fd, bd = frames.to(dev), full.to(dev)
    bytes_in = frames.numel()
    for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        for aa in (True, False):
            out = torch.empty(n, t, c, s, s, dtype=dtype, device=dev)
            run = be.roi_resize(fd, lut, bd, out, aa)
            st = torch.cuda.current_stream().cuda_stream
            ms = cuda_ms(lambda: run(st), 50, 5)
            nbytes = bytes_in + out.numel() * out.element_size()
            key = f"roi_resize_{tag}_{'aa' if aa else 'linear'}"
            res[key + "_us"] = round(ms * 1e3, 1)
            res[key + "_MB"] = round(nbytes / 1e6, 1)
            res[key + "_hbm_frac"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)

    # 1b. the colour jitter alone, in place on the three colour planes of a resident float clip
    if args.jitter:
        from video_classification_amd.input_pipeline import draw_color_jitter
        st = torch.cuda.current_stream().cuda_stream
        for tag, nn, ch, dtype, bgr, mean, std in (("v2_f32", n, 7, torch.float32, False, 0.0, 1.0),
                                                   ("v2_bf16", n, 7, torch.bfloat16, False, 0.0, 1.0),
                                                   ("htah_f32", 55, 21, torch.float32, True, 0.45, 0.225)):
            clip = ((torch.rand(nn, t, ch, s, s, device=dev) - mean) / std).to(dtype)
            ws = torch.empty(be.color_jitter_workspace_bytes(nn, t, s, s) // 4, device=dev)
            prm = draw_color_jitter(nn, generator=g)
            nbytes = 3 * 3 * nn * t * s * s * clip.element_size()
            for sub, p in (("", prm), ("_nocontrast", torch.where(prm == 1.0, torch.tensor(-1.0), prm))):
                p = p.clone()
                p[:, 4:] = prm[:, 4:]
                run = be.color_jitter(clip, p.to(dev), ws, 0, bgr, mean, std)
                ms = cuda_ms(lambda: run(st), 50, 5)
                key = f"jitter_{tag}{sub}"
                res[key + "_us"] = round(ms * 1e3, 1)
                if not sub:
                    res[key + "_MB"] = round(nbytes / 1e6, 1)
                    res[key + "_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            del clip

    # 2. a host-fed v2 step: uint8 frames + boxes against the float batch resized on the host
    cfg = get_cfg()
    cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN, cfg.MODEL.INPUT_SIZE, cfg.MODEL.DTYPE = n, t, s, "bf16"
    mm = v2.ModelManager(cfg, dev)
    model = mm.init_model()
    from video_classification_amd.train import TrainStep
    step = TrainStep(model.engine, lr=1e-3, optimizer="sgd", momentum=0.9)
    boxes = torch.tensor([[20 + i, 10, 260 + i, 225] for i in range(n)], dtype=torch.int32)
    labels = torch.randint(0, 249, (n,), generator=g)
    ub = {"frames_u8": frames.pin_memory(), "box": boxes, "label": labels}
    X = torch.stack([F.interpolate(frames[i, :, 10:225, 20 + i:260 + i].permute(0, 3, 1, 2).float().div(255), (s, s),
                                   mode="bilinear", align_corners=False, antialias=True) for i in range(n)])
    fb = {"rgb": X[:, :, 0:3].contiguous().pin_memory(), "uv": X[:, :, 3:5].contiguous().pin_memory(),
          "flow": X[:, :, 5:7].contiguous().pin_memory(), "label": labels}
    model.train()
    runs = [("uint8", ub), ("float", fb)]
    if args.jitter:
        runs.append(("uint8_jitter", dict(ub, jitter=draw_color_jitter(n, generator=g).pin_memory())))
    for tag, batch in runs:
        def one():
            x, y = mm.prepare_data(batch)
            step(x[0], x[1], y)
        for _ in range(args.warmup):
            one()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one()
        torch.cuda.synchronize()
        res[f"step_{tag}_ms"] = round((time.perf_counter() - t0) * 1e3 / args.steps, 2)
        res[f"step_{tag}_peak_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)

    # 3. what the loader no longer does: one clip's F.interpolate on one host thread
    torch.set_num_threads(1)
    clip = frames[0, :, 10:225, 20:260].permute(0, 3, 1, 2).float().div(255)
    t0 = time.perf_counter()
    for _ in range(3):
        F.interpolate(clip, (s, s), mode="bilinear", align_corners=False, antialias=True)
    res["host_resize_clip_ms"] = round((time.perf_counter() - t0) * 1e3 / 3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
