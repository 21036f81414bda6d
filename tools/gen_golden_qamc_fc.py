#!/usr/bin/env python3
"""Generate tests/golden/qamc_fc.npz by running the REFERENCE's own `VIOLET_QAMC` (main_qamc.py:50-103) on CPU in fp32.

Tiny Video-Swin, T = 4 frames of 224^2, B = 2 clips, O = 3 options; weights and inputs are the closed-form tensors of oracle/violet_ref.py
(`cfg["task"] = "retrieval"` gives the `fc` shapes), the option texts are the oracle's batch of B * O sequences viewed (B, O, X).

* default model (num_video_tokens = -1), eval mode: the logits, CrossEntropyLoss against ANS and its backward -- sampled fc.* gradients,
  the global gradient norm, the names whose .grad stays None -- the same backward seeded with a fixed generic d(logits) PROBE_DL
  (sampled fc.* gradients and the norm), and per clip the arg-max option with its top-2 logit margin.
* num_video_tokens = 48, eval mode: vid_key / vid_query = VID_SCALE x the oracle's closed form of their names (the formula, not 1.2 M
  floats, travels: tests rebuild them).  F.gumbel_softmax is wrapped to add a noise tensor chosen here instead of its own draw: the
  heads h % 3 == 0 get one decisive spike, the others zero noise so the column sums decide.  Recorded: the noise, the column sums c
  the wrapper received, the per-head arg-max, the `context_mask` select_vid_token returned, the logits, and per head its top-2 margin
  of c + g.
* the state-dict key lists of both reference models.
Needs the reference tree (build container only, like tools/gen_goldens.py).

    python tools/gen_golden_qamc_fc.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_goldens as G  # noqa: E402  (stubs, reference import recipe, ref_args)
from oracle import violet_ref as R  # noqa: E402

T_FRAMES, B, O = 4, 2, 3
ANS = [1, 2]
NTOK = 48
PROBE_DL = [[0.7, -0.4, 0.2], [-0.3, 0.5, 0.9]]
VID_SCALE = 10.0                      # vid_* = VID_SCALE * R.closed_form(name, (768, 768)): std 0.2, column sums of order 1 apart


def vid_weights(H=768):
    return {k: VID_SCALE * R.closed_form(k, (H, H)) for k in ("vid_key.weight", "vid_query.weight")}


def make_inputs(cfg):
    img, _, _ = R.make_batch(cfg, B)
    _, txt, mask = R.make_batch(cfg, B * O)
    return img, txt.view(B, O, -1), mask.view(B, O, -1)


def build(mq, cfg, ntok):
    args = G.ref_args("tiny", T_FRAMES, mvm_target="pixel")
    args.update(num_video_tokens=ntok, gumble_tau=1.0, size_option=O)
    model = mq.VIOLET_QAMC(args, None).eval()

    def mask_ext(m, shape=None, device=None):                     # transformers 4.26 semantics, as tools/gen_goldens.py
        m = m[:, None, None, :] if m.dim() == 2 else m[:, None, :, :]
        return (1.0 - m.float()) * torch.finfo(torch.float32).min
    model.mask_ext = mask_ext
    enc_fwd = model.trsfr.forward

    def trsfr_forward(feat, mask=None, output_attentions=False, **kw):
        o = enc_fwd(feat, attention_mask=mask)
        return {"last_hidden_state": (o[0] if not hasattr(o, "last_hidden_state") else o.last_hidden_state), "attentions": ()}
    model.trsfr.forward = trsfr_forward
    sd = R.make_state_dict(cfg)
    if ntok != -1:
        sd.update(vid_weights())
    own = model.state_dict()
    miss = [k for k in own if k not in sd and "relative_position_index" not in k]
    assert not miss, miss[:8]
    model.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    return model


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    G.import_reference()
    import main_qamc as mq
    cfg = R.make_cfg("tiny", T=T_FRAMES)
    cfg["task"] = "retrieval"
    img, txt, mask = make_inputs(cfg)
    ans = torch.tensor(ANS)
    d = dict(ans=ans.numpy(), T=np.array(T_FRAMES), B=np.array(B), O=np.array(O), ntok=np.array(NTOK), vid_scale=np.array(VID_SCALE))
    # ---- default model
    model = build(mq, cfg, -1)
    d["keys_default"] = np.array(sorted(model.state_dict().keys()))
    out, _ = model(img, txt, mask, ans)
    ls = torch.nn.CrossEntropyLoss()(out, ans)
    ls.backward()
    d["logits"] = out.detach().double().numpy()
    d["loss"] = np.array(float(ls.detach()))
    gsq, no_grad = 0.0, []
    for k, p_ in model.named_parameters():
        if p_.grad is None:
            no_grad.append(k)
            continue
        gsq += float((p_.grad.double() ** 2).sum())
        if k.startswith("fc."):
            G.put(d, "g." + k, p_.grad, 32)
    d["grad_norm"] = np.array(gsq ** 0.5)
    d["no_grad"] = np.array(no_grad)
    # the loss gradient is a ~24x cancellation here (a clip's O weights p - y sum to zero over nearly equal option gradients), a poor
    # probe of a bf16 backward: the same backward seeded with the fixed generic d(out) PROBE_DL is recorded as well
    model.zero_grad()
    out_p, _ = model(img, txt, mask, ans)
    (out_p * torch.tensor(PROBE_DL)).sum().backward()
    gsq_p = 0.0
    for k, p_ in model.named_parameters():
        if p_.grad is None:
            continue
        gsq_p += float((p_.grad.double() ** 2).sum())
        if k.startswith("fc."):
            G.put(d, "probe.g." + k, p_.grad, 32)
    d["probe.grad_norm"] = np.array(gsq_p ** 0.5)
    d["probe.dl"] = np.array(PROBE_DL)
    top = torch.topk(out.detach(), 2, dim=1)
    d["pred"] = top.indices[:, 0].numpy()
    d["pred_margin"] = (top.values[:, 0] - top.values[:, 1]).double().numpy()
    # ---- num_video_tokens = 48, eval mode, chosen noise
    model = build(mq, cfg, NTOK)
    d["keys_sel"] = np.array(sorted(model.state_dict().keys()))
    Lv = (1 + (224 // 32) ** 2) * T_FRAMES
    rec = {}
    orig_gs, orig_sel = torch.nn.functional.gumbel_softmax, model.select_vid_token

    def gumbel_fixed(logits, tau=1.0, hard=False, dim=-1, **kw):
        c = logits.detach()
        noise = torch.zeros_like(c)
        span = float(c.max() - c.min())
        for h in range(0, c.shape[1], 3):                       # one spike per clip and head: beats every column-sum difference
            j = (17 * h + 5) % c.shape[2]
            noise[:, h, j] = 2.0 * span + 1.0
        rec["c"], rec["noise"] = c.clone(), noise
        y_soft = ((logits + noise) / tau).softmax(dim)          # torch's gumbel_softmax with `gumbels` replaced by the chosen noise
        index = y_soft.max(dim, keepdim=True)[1]
        y_hard = torch.zeros_like(logits).scatter_(dim, index, 1.0)
        rec["idx"] = index.squeeze(dim)
        return y_hard - y_soft.detach() + y_soft

    def select(feat_img, mask_img):
        cm = orig_sel(feat_img, mask_img)
        rec["context_mask"] = cm.detach().clone()
        return cm
    model.select_vid_token = select
    torch.nn.functional.gumbel_softmax = gumbel_fixed
    try:
        with torch.no_grad():
            out_s, _ = model(img, txt, mask, ans)
    finally:
        torch.nn.functional.gumbel_softmax = orig_gs
    c, g = rec["c"], rec["noise"]
    assert c.shape == (B, NTOK, Lv), c.shape
    s2 = torch.topk(c + g, 2, dim=-1).values
    d["sel.noise"] = g.float().numpy()
    d["sel.c"] = c.double().numpy()
    d["sel.idx"] = rec["idx"].numpy().astype(np.int32)
    d["sel.margin"] = (s2[..., 0] - s2[..., 1]).double().numpy()
    d["sel.context_mask"] = rec["context_mask"].numpy().astype(np.uint8)
    d["sel.logits"] = out_s.double().numpy()
    np.savez_compressed(os.path.join(G.OUT, "qamc_fc.npz"), **d)
    print("qamc_fc ok probe gn", gsq_p ** 0.5, "logits", out.detach().numpy().round(4).tolist(), "loss", float(ls), "gn", gsq ** 0.5, "no_grad", no_grad)
    print("  sel: logits", out_s.numpy().round(4).tolist(), "tokens kept", rec["context_mask"].sum(1).tolist(),
          "heads with margin > 0.25:", int((d["sel.margin"] > 0.25).sum()), "of", B * NTOK,
          "(zero-noise heads:", int((d["sel.margin"][:, [h for h in range(NTOK) if h % 3]] > 0.25).sum()), ")")


if __name__ == "__main__":
    main()
