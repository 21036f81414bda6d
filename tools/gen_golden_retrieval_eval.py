#!/usr/bin/env python3
"""Generate tests/golden/retrieval_eval.npz by running the REFERENCE's own `VIOLET_RetrievalEval` (eval_retrieval.py) on CPU in fp32.

Corpus: 3 videos of 2 clips each and 4 texts; video 0 holds texts 0 and 2.  The four (text, video) items go through
`forward(typ='feat')` once (clip mean of the video features, the text features), the video bank keeps the first occurrence of every
video id in order of appearance (eval_retrieval_tsv.py:53-58), and all 4 x 3 (text, video) pairs of the bank go through
`forward(typ='cross')` in one batch, text-major.  Weights and inputs are the closed-form tensors of oracle/violet_ref.py, so the
fixture holds outputs only.  Needs the reference tree (build container only, like tools/gen_goldens.py).

    python tools/gen_golden_retrieval_eval.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_goldens as G  # noqa: E402  (stubs, reference import recipe, ref_args)
from oracle import violet_ref as R  # noqa: E402

T_FRAMES, CLIPS = 4, 2
ITEMS = [(0, 0), (1, 1), (2, 0), (3, 2)]          # (text id, video id) in dataset order: video 0 holds texts 0 and 2


def corpus(cfg):
    """-> img (4, CLIPS, T, 3, S, S) per item, txt / mask (4, X), the video bank's ids in order of first appearance, gt bank index per text"""
    clips, _, _ = R.make_batch(cfg, 3 * CLIPS)                    # clip c of video v = row v * CLIPS + c
    clips = clips.view(3, CLIPS, *clips.shape[1:])
    _, txt, mask = R.make_batch(cfg, len(ITEMS))
    img = torch.stack([clips[v] for _, v in ITEMS])
    bank = []
    for _, v in ITEMS:
        if v not in bank:
            bank.append(v)
    gt = np.array([bank.index(v) for _, v in ITEMS], dtype=np.int32)
    return img, txt, mask, bank, gt


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    G.import_reference()
    import eval_retrieval as er
    cfg = R.make_cfg("tiny", T=T_FRAMES)
    cfg["task"] = "retrieval"
    sd = R.make_state_dict(cfg)
    args = G.ref_args("tiny", T_FRAMES, mvm_target="pixel")
    model = er.VIOLET_RetrievalEval(args, None).eval()

    def mask_ext(m, shape=None, device=None):                     # transformers 4.26 semantics, as tools/gen_goldens.py
        m = m[:, None, None, :] if m.dim() == 2 else m[:, None, :, :]
        return (1.0 - m.float()) * torch.finfo(torch.float32).min
    model.mask_ext = mask_ext
    enc_fwd = model.trsfr.forward

    def trsfr_forward(feat, mask=None, output_attentions=False, **kw):
        o = enc_fwd(feat, attention_mask=mask)
        return {"last_hidden_state": (o[0] if not hasattr(o, "last_hidden_state") else o.last_hidden_state), "attentions": ()}
    model.trsfr.forward = trsfr_forward
    own = model.state_dict()
    miss = [k for k in sd if k not in own]
    assert not miss, miss[:8]
    model.load_state_dict(sd, strict=False)
    img, txt, mask, bank, gt = corpus(cfg)
    with torch.no_grad():
        feat_img, mask_img, feat_txt, mask_txt = model(typ="feat", img=img, txt=txt, mask=mask)
        first = [[v for _, v in ITEMS].index(b) for b in bank]  # item index of each bank video's first occurrence
        vb, mb = feat_img[first], mask_img[first]
        nt, nv = len(ITEMS), len(bank)
        ti = torch.arange(nt).repeat_interleave(nv)
        vi = torch.arange(nv).repeat(nt)
        out = model(typ="cross", feat_img=vb[vi], mask_img=mb[vi], feat_txt=feat_txt[ti], mask_txt=mask_txt[ti])
        logits = out.view(nt, nv)
        scores = torch.sigmoid(logits.float())
    d = dict(logits=logits.double().numpy(), scores=scores.double().numpy(), gt=gt, bank=np.array(bank, dtype=np.int32),
             items=np.array(ITEMS, dtype=np.int32), T=np.array(T_FRAMES), clips=np.array(CLIPS))
    G.put(d, "feat_img", vb, 64)
    G.put(d, "feat_txt", feat_txt, 64)
    d["mask_img"] = mb.numpy().astype(np.int64)
    np.savez_compressed(os.path.join(G.OUT, "retrieval_eval.npz"), **d)
    print("retrieval_eval ok logits", logits.numpy().round(4).tolist())


if __name__ == "__main__":
    main()
