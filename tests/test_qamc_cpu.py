"""fc-head multiple-choice video QA (VIOLET_QAMC, main_qamc.py:50-155) without a GPU: the task's parameter inventory and options, the
checkpoint key lists of the reference's two models, the optimizer runs of Agent_QAMC, a CPU restatement from oracle functions that
pins tests/golden/qamc_fc.npz (tools/gen_golden_qamc_fc.py) to the oracle, and the host checks of vmvm_video_token_select."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import violet_ref as R
from pytorch_empirical_mvm_amd import config as CFG

G = os.path.join(os.path.dirname(__file__), "golden")
H = 768


def _args(**kw):
    return CFG.get_args(vis_backbone_size="tiny", size_frame=4, max_size_frame=6, task="qamc", mvm_target=[], **kw)


def _fixture():
    return np.load(os.path.join(G, "qamc_fc.npz"))


def _rpi_names(cfg):
    return {f"enc_img.swin.layers.{i}.blocks.{b}.attn.relative_position_index" for i, d in enumerate(cfg["depths"]) for b in range(d)}


def test_param_shapes_with_and_without_token_selection():
    base = CFG.param_shapes(CFG.model_cfg(_args()))
    ret = CFG.param_shapes(CFG.model_cfg(CFG.get_args(vis_backbone_size="tiny", size_frame=4, max_size_frame=6, task="retrieval", mvm_target=[])))
    assert {k: tuple(v) for k, v in base.items()} == {k: tuple(v) for k, v in ret.items()}       # the fc shapes of retrieval
    assert tuple(base["fc.1.weight"]) == (2 * H, H) and tuple(base["fc.3.weight"]) == (1, 2 * H) and tuple(base["fc.3.bias"]) == (1,)
    assert not any(k.startswith(("vid_", "fc_mtm", "decoder_")) for k in base)
    for n in (48, 96, 192):
        s = CFG.param_shapes(CFG.model_cfg(_args(num_video_tokens=n)))
        assert set(s) - set(base) == {"vid_key.weight", "vid_query.weight"}
        assert tuple(s["vid_key.weight"]) == (H, H) and tuple(s["vid_query.weight"]) == (H, H)
    cfg = CFG.model_cfg(_args())
    assert (cfg["num_video_tokens"], cfg["gumble_tau"], cfg["size_option"]) == (-1, 1.0, 5)
    assert "num_video_tokens" not in CFG.DEFAULT_ARGS and "num_video_tokens" not in CFG.model_cfg(CFG.get_args())


@pytest.mark.parametrize("kw", [dict(num_video_tokens=64), dict(num_video_tokens=0), dict(num_video_tokens=-2), dict(gumble_tau=0.0),
                                dict(gumble_tau=-1.0), dict(gumble_tau=float("nan")), dict(size_option=0)])
def test_invalid_options_are_rejected(kw):
    with pytest.raises(ValueError):
        CFG.model_cfg(_args(**kw))
    with pytest.raises(ValueError):
        CFG.qamc_options(_args(**kw))


def test_state_dict_keys_equal_the_reference_models():
    d = _fixture()
    for n, name in ((-1, "keys_default"), (48, "keys_sel")):
        cfg = CFG.model_cfg(_args(num_video_tokens=n))
        mine = set(CFG.param_shapes(cfg)) | _rpi_names(cfg)
        assert mine == set(d[name].tolist()), (name, sorted(mine ^ set(d[name].tolist()))[:8])
    assert d["no_grad"].tolist() == ["enc_img.emb_odr"]


def test_selection_weights_are_frozen_and_fc_is_the_tail_of_the_other_segments():
    """ParamStore layout of the qamc task: vid_* in the frozen segment (no gradient, no AdamW, no decay), fc.* the tail of segments
    1 / 3; Agent_QAMC.segment_runs: base rate on the rest, lr * vis_backbone_lr_mul on the fc.* run, Swin segments at the base rate."""
    from pytorch_empirical_mvm_amd.downstream import Agent_QAMC
    from pytorch_empirical_mvm_amd.store import ParamStore
    from pytorch_empirical_mvm_amd.agent import Agent_Pretrain
    arch = dict(embed_dim=32, depths=(1, 1, 1, 1), num_heads=(1, 2, 4, 8), window=(8, 7, 7))
    args = _args(num_video_tokens=48, arch_override=arch, bert_layers=2, vis_backbone_lr_mul=10)
    S = ParamStore(CFG.param_shapes(CFG.model_cfg(args)), torch.device("cpu"))
    fa, fe = S.segments[4]
    for n in ("vid_key.weight", "vid_query.weight"):
        o, c, _ = S.index[n]
        assert fa <= o and o + c <= fe and o + c <= S.total
    assert S.n_trainable == S.segments[3][1] <= fa
    tails = {gi: S.tail_start(gi, "fc.") for gi in (1, 3)}
    assert tails[1] == S.index["fc.1.weight"][0] and tails[3] == S.index["fc.1.bias"][0]
    assert S.tail_start(0, "fc.") == S.segments[0][1]                    # none in a Swin segment
    with pytest.raises(AssertionError):
        S.tail_start(1, "trsfr.")                                          # not a tail
    stub = types.SimpleNamespace(engine=types.SimpleNamespace(store=S), _fc_tail=tails, args=args, sched_step=50)
    lrs = Agent_QAMC.current_lrs(stub)
    assert lrs[0] == pytest.approx(10 * lrs[1]) and lrs[2] == lrs[0] and lrs[3] == lrs[1]
    for gi in range(4):
        runs = Agent_QAMC.segment_runs(stub, gi, lrs)
        a, e = S.segments[gi]
        assert runs[0][0] == a and runs[-1][1] == e and all(r[1] == s[0] for r, s in zip(runs, runs[1:]))
        for ra, re_, lr in runs:
            names = [n for n, (o, c, _) in S.index.items() if ra <= o < re_]
            assert names and all(n.startswith("fc.") == (lr == lrs[0] and gi in (1, 3) and ra == tails[gi]) for n in names), (gi, ra)
    assert Agent_Pretrain.segment_runs(stub, 1, lrs) == [(S.segments[1][0], S.segments[1][1], lrs[1])]      # the other agents: one run


def _fc(sd, x):
    x = F.relu(F.linear(x, sd["fc.1.weight"], sd["fc.1.bias"]))
    return F.linear(x, sd["fc.3.weight"], sd["fc.3.bias"]).squeeze(-1)


def _select_restated(feat_img, mask_img, wk, wq, n, noise):
    """select_vid_token (main_qamc.py:66-83) in plain torch, eval mode, with `noise` in place of the gumbel draw"""
    B, Lv, Hd = feat_img.shape
    d_ = Hd // n
    k = F.linear(feat_img, wk).view(B, Lv, n, d_).permute(0, 2, 1, 3)
    q = F.linear(feat_img, wq).view(B, Lv, n, d_).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) / math.sqrt(Hd) + ((1.0 - mask_img.float()) * torch.finfo(torch.float32).min)[:, None, None, :]
    c = s.softmax(-1).sum(-2)
    idx = (c + noise).argmax(-1)
    hard = torch.zeros_like(c).scatter_(-1, idx[..., None], 1.0).sum(1)
    return c, idx, mask_img * (hard > 0)


@pytest.fixture(scope="module")
def oracle_run():
    d = _fixture()
    T, B, O = int(d["T"]), int(d["B"]), int(d["O"])
    cfg = R.make_cfg("tiny", T=T)
    cfg["task"] = "retrieval"
    sd = R.make_state_dict(cfg)
    img, _, _ = R.make_batch(cfg, B)
    _, txt, mask = R.make_batch(cfg, B * O)
    with torch.no_grad():
        feat_img, mask_img = R.enc_video(sd, cfg, img)
        feat_txt = R.enc_txt(sd, txt)
    return d, cfg, sd, feat_img, mask_img, feat_txt, mask, (T, B, O)


def test_oracle_restatement_reproduces_the_fixture(oracle_run):
    """enc_video / enc_txt / go_cross / fc of the oracle reproduce the reference's logits and loss; with the fixture's noise the torch
    restatement of select_vid_token reproduces its column sums, arg-maxes, context mask, and the logits of that model"""
    d, cfg, sd, feat_img, mask_img, feat_txt, mask, (T, B, O) = oracle_run
    Lv = feat_img.shape[1]
    ii = [b for b in range(B) for _ in range(O)]
    with torch.no_grad():
        out = R.go_cross(sd, cfg, feat_img[ii], mask_img[ii], feat_txt, mask)
        lg = _fc(sd, out[:, Lv]).view(B, O)
    assert np.abs(lg.double().numpy() - d["logits"]).max() <= 1e-4, (lg, d["logits"])
    ls = F.cross_entropy(lg, torch.from_numpy(d["ans"]))
    assert abs(float(ls) - float(d["loss"])) <= 1e-4
    n, scale = int(d["ntok"]), float(d["vid_scale"])
    wk, wq = scale * R.closed_form("vid_key.weight", (H, H)), scale * R.closed_form("vid_query.weight", (H, H))
    noise = torch.from_numpy(d["sel.noise"])
    with torch.no_grad():
        c, idx, cm = _select_restated(feat_img, mask_img, wk, wq, n, noise)
    assert c.shape == (B, n, Lv)
    assert np.abs(c.double().numpy() - d["sel.c"]).max() <= 1e-3 * max(1.0, float(np.abs(d["sel.c"]).max()))
    dec = d["sel.margin"] > 1e-3                          # (the restatement's f32 sums may reorder an exact near-tie)
    assert dec.mean() > 0.9
    assert np.array_equal(idx.numpy()[dec], d["sel.idx"][dec])
    assert np.array_equal(cm.numpy().astype(np.uint8), d["sel.context_mask"])
    with torch.no_grad():
        out = R.go_cross(sd, cfg, feat_img[ii], cm[ii], feat_txt, mask)
        lg_s = _fc(sd, out[:, Lv]).view(B, O)
    assert np.abs(lg_s.double().numpy() - d["sel.logits"]).max() <= 1e-4
    # the fixture's heads: one in three carries a decisive noise spike, the others are decided by the column sums alone
    spiked = (d["sel.noise"] != 0).any(-1)
    assert spiked[:, ::3].all() and not spiked[:, 1::3].any() and not spiked[:, 2::3].any()


def test_video_token_select_rejects_invalid_arguments_on_the_host():
    from pytorch_empirical_mvm_amd import lib
    l = lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    z = None
    f = l.vmvm_video_token_select
    ok = (p, p, z, z, 2, 250, H, 48, 0.1, 1, 0, 1, 0, p, p, z)

    def call(**kw):
        a = list(ok)
        names = ["q", "k", "mask", "noise", "B", "Lv", "H", "n", "p", "sd", "od", "sn", "on", "idx", "sel", "stream"]
        for key, v in kw.items():
            a[names.index(key)] = v
        return f(*a)
    for kw in (dict(q=z), dict(k=z), dict(idx=z), dict(sel=z), dict(n=100), dict(n=384), dict(n=24), dict(n=0), dict(H=0), dict(B=0),
               dict(Lv=0), dict(Lv=897), dict(p=1.0), dict(p=-0.01), dict(p=float("nan")), dict(q=p + 1), dict(k=p + 1)):
        assert call(**kw) == -1, kw
    assert l.vmvm_last_hip_error() == 0
