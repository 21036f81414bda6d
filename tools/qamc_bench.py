#!/usr/bin/env python3
"""fc-head multiple-choice video QA (VIOLET_QAMC / Agent_QAMC) at the tgif-action shape of _args/args_tgif-action.json: Video-Swin-B,
5 frames at 224^2 (Lv = 250), B = 8 clips, O = 5 options of X = 100 tokens (40 fusion sequences of 350 rows), 12 fusion layers,
seeded random weights and inputs.  For num_video_tokens = -1 and --ntok: the train step (forward, backward, AdamW; device events,
median), eval clips/s (step(is_train=False)), and for the selection the vmvm_video_token_select launch alone on the engine's own
projections (median of --reps launches, HIP events).  Prints one JSON line.

    python tools/qamc_bench.py [--steps 10] [--warmup 3] [--ntok 48] [--reps 50]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ntok", type=int, default=48, choices=[48, 96, 192])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--txt-len", type=int, default=100)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    from pytorch_empirical_mvm_amd import config as CFG
    from pytorch_empirical_mvm_amd import kernels as K
    from pytorch_empirical_mvm_amd.downstream import Agent_QAMC, VIOLET_QAMC
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    B, O, X, T = a.batch, a.options, a.txt_len, a.frames
    g = torch.Generator(device=dev).manual_seed(a.seed)
    img = torch.rand((B, T, 3, 224, 224), device=dev, generator=g) * 2.0 - 1.0
    txt = torch.randint(1000, 30000, (B, O, X), device=dev, generator=g)
    txt[:, :, 0] = 101
    lens = torch.randint(10, X + 1, (B, O, 1), device=dev, generator=g)
    mask = (torch.arange(X, device=dev)[None, None, :] < lens).long()
    ans = torch.randint(0, O, (B,), device=dev, generator=g)
    res = dict(tool="qamc_bench", B=B, O=O, X=X, frames=T, Lv=T * 50, steps=a.steps, warmup=a.warmup)
    for ntok in (-1, a.ntok):
        args = CFG.get_args(vis_backbone_size="base", size_frame=T, max_size_frame=max(T, 6), size_img=224, size_txt=X, size_option=O,
                            num_video_tokens=ntok, lr=2e-5, max_iter=1000, seed=a.seed)
        model = VIOLET_QAMC(args, None, device=dev)
        agent = Agent_QAMC(args, model)
        agent.sched_step = 100
        model.train()
        for _ in range(a.warmup):
            agent.step(img, txt, mask, ans, is_train=True)
        torch.cuda.synchronize()
        tr = _timed(lambda: agent.step(img, txt, mask, ans, is_train=True), a.steps)
        model.eval()
        for _ in range(max(1, a.warmup)):
            agent.step(img, txt, mask, ans, is_train=False)
        ev = _timed(lambda: agent.step(img, txt, mask, ans, is_train=False), a.steps)
        tag = "off" if ntok == -1 else f"on{ntok}"
        res[f"train_step_ms_{tag}"] = round(statistics.median(tr), 2)
        res[f"eval_clips_per_s_{tag}"] = round(B / (statistics.median(ev) / 1e3), 1)
        if ntok != -1:
            st = model.engine.qamc_select
            q, k = st["q"], st["k"]
            Lv = q.shape[0] // B
            sel = lambda: K.video_token_select(q, k, B, Lv, ntok, dropout_p=0.1, seed_drop=1, off_drop=0, seed_noise=1, off_noise=1 << 20)
            for _ in range(5):
                sel()
            us = [t * 1e3 for t in _timed(sel, a.reps)]
            res[f"select_us_{tag}"] = round(statistics.median(us), 1)
            res[f"select_us_{tag}_min"] = round(min(us), 1)
            res["tokens_kept_mean"] = round(float(st["sel"].float().sum(1).mean()), 1)
        del agent, model
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
