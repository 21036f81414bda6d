"""Full-corpus text-to-video retrieval evaluation on the HIP path (VIOLET_RetrievalEval, engine.retrieval_corpus_scores): the reference's
'feat' / 'cross' forms against retrieval_eval.npz (tools/gen_golden_retrieval_eval.py), the device pair loop against the aligned
'cross' form, the rank kernel's tie rule, bounded memory of the pair phase and the inference form of the fusion layer."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1.75e-2                       # bf16 rounding of the [CLS] state on the fc logits (as test_retrieval_pairs_scores_loss_and_step)


def _model(T=4, bert_layers=12):
    from oracle import violet_ref as R
    from pytorch_empirical_mvm_amd import config as CFG
    from pytorch_empirical_mvm_amd.downstream import VIOLET_RetrievalEval
    cfg = R.make_cfg("tiny", T=T, bert_layers=bert_layers)
    cfg["task"] = "retrieval"
    args = CFG.get_args(vis_backbone_size="tiny", size_frame=T, max_size_frame=6, bert_layers=bert_layers)
    model = VIOLET_RetrievalEval(args, None, device="cuda")
    _, unexpected = model.load_state_dict(R.make_state_dict(cfg))
    assert not unexpected, unexpected[:5]
    return model.eval(), cfg


@pytest.fixture(scope="module")
def golden_model():
    return _model()


@pytest.fixture(scope="module")
def small_model():
    return _model(bert_layers=2)


def _rank_rule(s, gt):
    """stable sort by descending score, 1-based position of gt (eval_retrieval_tsv.py:81-83)"""
    out = []
    for t in range(s.shape[0]):
        order = sorted(range(s.shape[1]), key=lambda v: -s[t, v])
        out.append(order.index(int(gt[t])) + 1)
    return np.array(out, dtype=np.int32)


def _samples_close(got, d, name, rel=2e-2, atol=2e-2):
    f = got.detach().double().cpu().flatten().numpy()
    assert tuple(got.shape) == tuple(d[name + ".shape"]), (got.shape, d[name + ".shape"])
    want = d[name + ".val"]
    err = np.abs(f[d[name + ".idx"]] - want)
    assert (err <= rel * np.abs(want) + atol).all(), (name, err.max())


def test_feat_and_cross_against_the_reference(golden_model):
    from oracle import violet_ref as R
    model, cfg = golden_model
    d = np.load(os.path.join(G, "retrieval_eval.npz"))
    items, clips = [tuple(x) for x in d["items"].tolist()], int(d["clips"])
    cl, _, _ = R.make_batch(cfg, 3 * clips)
    cl = cl.view(3, clips, *cl.shape[1:])
    _, txt, mask = R.make_batch(cfg, len(items))
    img = torch.stack([cl[v] for _, v in items])
    feat_img, mask_img, feat_txt, mask_txt = model(typ="feat", img=img, txt=txt, mask=mask)
    bank = d["bank"].tolist()
    first = [[v for _, v in items].index(b) for b in bank]
    vb, mb = feat_img[first], mask_img[first]
    _samples_close(vb, d, "feat_img")
    _samples_close(feat_txt, d, "feat_txt")
    assert np.array_equal(mb.cpu().numpy(), d["mask_img"])
    nt, nv = len(items), len(bank)
    ti = torch.arange(nt).repeat_interleave(nv).cuda()
    vi = torch.arange(nv).repeat(nt).cuda()
    lg = model(typ="cross", feat_img=vb[vi], mask_img=mb[vi], feat_txt=feat_txt[ti], mask_txt=mask_txt[ti])
    assert lg.shape == (nt * nv,)
    assert np.abs(lg.double().cpu().numpy() - d["logits"].reshape(-1)).max() <= TOL, (lg, d["logits"])
    # the corpus entry on the same items (two batches): banks, scores and the metric strings (ranks are not asserted here: the
    # closed-form weights give near-tied scores that bf16 may reorder)
    tids = list(range(nt))
    vids = [v for _, v in items]
    batches = [(img[:2], txt[:2], mask[:2], tids[:2], vids[:2]), (img[2:], txt[2:], mask[2:], tids[2:], vids[2:])]
    out = model.evaluate_corpus(batches, {t: v for t, v in zip(tids, vids)})
    assert out["vid_ids"] == bank and out["txt_ids"] == tids
    assert np.abs(out["scores"].double().cpu().numpy() - d["scores"]).max() <= TOL / 4          # sigmoid' <= 1/4
    assert set(out["metrics"]) == {"r@1", "r@5", "r@10", "median"} and out["ranks"].dtype == torch.int32
    assert np.array_equal(out["ranks"].numpy(), _rank_rule(out["scores"].cpu().numpy(), d["gt"]))


def test_corpus_pairs_equal_the_aligned_cross_form(small_model):
    model, cfg = small_model
    eng = model.engine
    Nt, Nv, Lv, X, Hd = 7, 5, 4 * 50, 32, 768
    g = torch.Generator().manual_seed(3)
    vid = (torch.randn(Nv, Lv, Hd, generator=g) * 0.8).to(torch.bfloat16).cuda()
    txt = (torch.randn(Nt, X, Hd, generator=g) * 0.8).to(torch.bfloat16).cuda()
    tmask = torch.zeros(Nt, X, dtype=torch.long)
    for t in range(Nt):
        tmask[t, :6 + 3 * t] = 1
    tmask = tmask.cuda()
    gt = [t % Nv for t in range(Nt)]
    ti = torch.arange(Nt).repeat_interleave(Nv).cuda()
    vi = torch.arange(Nv).repeat(Nt).cuda()
    lg = model(typ="cross", feat_img=vid[vi], mask_img=torch.ones(Nt * Nv, Lv, dtype=torch.long, device="cuda"), feat_txt=txt[ti],
               mask_txt=tmask[ti]).view(Nt, Nv)
    want = torch.sigmoid(lg.float()).cpu().numpy()
    Lq = Lv + X
    from pytorch_empirical_mvm_amd.engine_downstream import plan_retrieval_blocks
    for max_rows in (2 * Nv * Lq, 3 * Lq):                         # 2 texts x all videos (4 blocks, the last one short); 1 text x 3 | 2 videos
        kinds = {nv == Nv for _, _, _, nv in plan_retrieval_blocks(Nt, Nv, Lq, max_rows)}
        assert len(kinds) == 1
        scores, ranks = eng.retrieval_corpus_scores(vid, txt, tmask, gt, max_rows=max_rows)
        s = scores.cpu().numpy()
        assert np.abs(s - want).max() <= TOL / 4, (max_rows, np.abs(s - want).max())
        assert np.array_equal(ranks.numpy(), _rank_rule(s, gt))


def test_feat_clip_mean_equals_single_clip_go_feat(small_model):
    from oracle import violet_ref as R
    model, cfg = small_model
    B, Cl = 2, 3
    imgs, txt, mask = R.make_batch(cfg, B * Cl)
    img = imgs.view(B, Cl, *imgs.shape[1:])
    txt, mask = txt[:B], mask[:B]
    fi, mi, ft, mt = model(typ="feat", img=img, txt=txt, mask=mask)
    acc = 0
    for c in range(Cl):
        f1, m1, t1, _ = model.go_feat(img[:, c].contiguous(), txt, mask)
        acc = acc + f1.float()
    ref = acc / Cl
    assert fi.shape == ref.shape and mi.shape == m1.shape and bool((mi == 1).all())
    assert (fi.float() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item() + 1e-3
    assert (ft.float() - t1.float()).abs().max().item() <= 1e-2


def test_rank_kernel_tie_rule_and_saturation():
    from pytorch_empirical_mvm_amd import kernels as K
    rng = np.random.default_rng(5)
    Nt, Nv = 9, 1000
    lg = rng.choice(np.array([-3.0, -0.5, 0.0, 0.5, 2.0, 20.0, 25.0, 40.0], dtype=np.float32), size=(Nt, Nv))   # exact ties, saturation
    lg[0] = 30.0                                                                    # a whole row saturated: rank = gt + 1
    lg[1, :] = rng.standard_normal(Nv).astype(np.float32)
    gt = np.array([417, 3, 999, 0, 128, 255, 256, 700, 64], dtype=np.int32)
    s = torch.from_numpy(lg).cuda()
    rank = K.retrieval_rank(s, torch.from_numpy(gt).cuda())
    sc = s.cpu().numpy()
    assert (sc[lg >= 20.0] == 1.0).all()
    assert np.abs(sc - 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))).max() <= 1e-6
    got = rank.cpu().numpy()
    assert got[0] == gt[0] + 1
    assert np.array_equal(got, _rank_rule(sc, gt)), (got, _rank_rule(sc, gt))


def test_pair_phase_memory_does_not_grow_with_the_corpus(small_model):
    model, cfg = small_model
    eng = model.engine
    Lv, X, Hd = 200, 32, 768
    Lq = Lv + X
    max_rows = 16 * Lq                                           # 8 x 8: 2 texts x 8 videos; 32 x 32: 1 text x 16 videos -- 16 sequences each

    def run(n):
        vid = torch.randn(n, Lv, Hd, device="cuda").to(torch.bfloat16)
        txt = torch.randn(n, X, Hd, device="cuda").to(torch.bfloat16)
        tm = torch.ones(n, X, dtype=torch.long, device="cuda")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        scores, _ = eng.retrieval_corpus_scores(vid, txt, tm, list(range(n)), max_rows=max_rows)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return peak, vid.numel() * 2 + txt.numel() * 2 + scores.numel() * 4

    run(8)                                                       # warm-up: cached index tensors of the query-row layer
    p8, _ = run(8)
    p32, corpus32 = run(32)
    assert p32 - p8 <= corpus32, (p8, p32, corpus32)
    assert p32 < 32 * 32 * Lq * Hd * 2, (p32,)                   # far below one pass over all 1 024 sequences


def test_inference_layer_form_is_bit_identical(small_model):
    from pytorch_empirical_mvm_amd.store import V, NoTape
    model, cfg = small_model
    eng = model.engine
    assert eng.sw.block_abi
    nseq, Lq, Hd = 3, 232, 768
    x = (torch.randn(nseq * Lq, Hd, device="cuda") * 0.5).to(torch.bfloat16)
    km = torch.ones(nseq, Lq, dtype=torch.uint8, device="cuda")
    km[1, 220:] = 0
    saved = eng.tape
    try:
        eng.tape = []
        with_codes = eng._bert_layer_block(V(x), nseq, Lq, km, 0, False).t.clone()
        eng.tape = NoTape()
        no_codes = eng._bert_layer_block(V(x), nseq, Lq, km, 0, False).t.clone()
    finally:
        eng.tape = saved
    torch.cuda.synchronize()
    assert torch.equal(with_codes, no_codes)
