#!/usr/bin/env python3
"""Full-corpus text-to-video retrieval evaluation on a synthetic corpus (VIOLET_RetrievalEval / engine.retrieval_corpus_scores) at the
MSRVTT shape of args_msrvtt-retrieval.json: Video-Swin-B, 5 frames at 224^2 (Lv = 5 * (1 + 49) = 250), 25 text tokens, 12 fusion
layers, seeded random weights.  Prints one JSON line: bank-phase and pair-phase seconds (device events), pairs/s, the fusion-forward
FLOP of the pair phase from the shapes (`pair_flop` below) and TFLOP/s, peak device memory.

    python tools/retrieval_eval_bench.py [--texts 1000] [--videos 1000] [--clips 2] [--max-rows 262144] [--batch 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pair_flop(Lv, X, H=768, F=3072, layers=12, heads_dim_total=768):
    """fusion-forward FLOP of ONE (text, video) pair as the pair loop runs it (2 per multiply-add): layers 0 .. n-2 on all Lq rows (QKV,
    attention scores and context, output projection, FFN), the last layer's key / value projection on all rows and its query, attention,
    projections and FFN on the [CLS] row only, then fc (H -> 2H, 2H -> 1)"""
    Lq = Lv + X
    full_row = 2 * H * (3 * H + H + 2 * F) + 2 * 2 * Lq * heads_dim_total
    last = Lq * 2 * H * 2 * H + (2 * H * H + 2 * 2 * Lq * heads_dim_total + 2 * H * H + 2 * 2 * H * F)
    head = 2 * H * 2 * H + 2 * 2 * H
    return (layers - 1) * Lq * full_row + last + head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=1000)
    ap.add_argument("--videos", type=int, default=1000)
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--txt-len", type=int, default=25)
    ap.add_argument("--max-rows", type=int, default=None)
    ap.add_argument("--batch", type=int, default=10, help="items per encoder batch of the bank phase")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    from pytorch_empirical_mvm_amd import config as CFG
    from pytorch_empirical_mvm_amd.downstream import VIOLET_RetrievalEval
    from pytorch_empirical_mvm_amd.engine_downstream import RETRIEVAL_MAX_ROWS, plan_retrieval_blocks
    assert torch.cuda.is_available(), "needs a GPU"
    max_rows = a.max_rows or RETRIEVAL_MAX_ROWS
    args = CFG.get_args(vis_backbone_size="base", size_frame=a.frames, max_size_frame=max(a.frames, 6), size_img=224, size_txt=a.txt_len, seed=a.seed)
    model = VIOLET_RetrievalEval(args, None, device="cuda:0").eval()
    eng = model.engine
    Nt, Nv, X, T, Cl = a.texts, a.videos, a.txt_len, a.frames, a.clips
    Hd = eng.cfg["hidden"]
    Lv = T * (1 + 49)
    g = torch.Generator(device="cuda:0").manual_seed(a.seed)
    vid_bank = torch.empty((Nv, Lv, Hd), device="cuda:0", dtype=torch.bfloat16)
    txt_bank = torch.empty((Nt, X, Hd), device="cuda:0", dtype=torch.bfloat16)
    txt_mask = torch.zeros((Nt, X), device="cuda:0", dtype=torch.uint8)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    # bank phase: item i = (video i % Nv, text i % Nt); one encoder pass per batch of items, `Cl` clips per video
    n_items = max(Nt, Nv)
    for i0 in range(0, n_items, a.batch):
        B = min(a.batch, n_items - i0)
        img = torch.rand((B, Cl, T, 3, 224, 224), device="cuda:0", generator=g) * 2.0 - 1.0
        txt = torch.randint(1000, 30000, (B, X), device="cuda:0", generator=g)
        lens = torch.randint(6, X + 1, (B, 1), device="cuda:0", generator=g)
        mask = (torch.arange(X, device="cuda:0")[None, :] < lens).long()
        fv, ft, km = eng.retrieval_encode_bank(img, txt, mask)
        for b in range(B):
            i = i0 + b
            if i < Nv:
                vid_bank[i].copy_(fv[b])
            if i < Nt:
                txt_bank[i].copy_(ft[b])
                txt_mask[i].copy_(km[b])
    e1.record()
    gt = [t % Nv for t in range(Nt)]
    scores, ranks = eng.retrieval_corpus_scores(vid_bank, txt_bank, txt_mask, gt, max_rows=max_rows)
    e2.record()
    torch.cuda.synchronize()
    bank_s, pair_s = e0.elapsed_time(e1) / 1e3, e1.elapsed_time(e2) / 1e3
    flop = pair_flop(Lv, X, Hd, layers=eng.cfg["bert_layers"]) * Nt * Nv
    blocks = plan_retrieval_blocks(Nt, Nv, Lv + X, max_rows)
    print(json.dumps(dict(tool="retrieval_eval_bench", texts=Nt, videos=Nv, clips=Cl, frames=T, Lv=Lv, X=X, Lq=Lv + X, max_rows=max_rows,
                          blocks=len(blocks), bank_s=round(bank_s, 3), pair_s=round(pair_s, 3), pairs_per_s=round(Nt * Nv / pair_s, 1),
                          pair_flop=flop, pair_tflops=round(flop / pair_s / 1e12, 1), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                          rank_min=int(ranks.min()), rank_max=int(ranks.max()), device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
