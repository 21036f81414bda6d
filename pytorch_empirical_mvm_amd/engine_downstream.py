"""Downstream passes of `VioletEngine` (engine.py): retrieval, open-ended QA, multiple-choice / MLM-generation QA.
Methods of the engine class."""
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import config as CFG
from . import kernels as K
from . import swin_index as SI
from .store import BF16, F32, V, DropScale, NoTape, _acc, _gout, _h2d, _dev_i32

RETRIEVAL_MAX_ROWS = 1 << 18            # default cap of P * Lq, the fusion rows of one block of the corpus evaluation


def plan_retrieval_blocks(Nt, Nv, Lq, max_rows=RETRIEVAL_MAX_ROWS):
    """Blocks (t0, nt, v0, nv) of the (Nt, Nv) pair grid for `retrieval_corpus_scores`: nt texts x all Nv videos when one text row fits
    (Nv * Lq <= max_rows), else one text x a range of nv videos (the ranges of a row as even as the cap allows).  Either way the pairs
    p = t * nv + v of a block are one contiguous run [t0 * Nv + v0, + nt * nv) of the row-major score matrix, and nt * nv * Lq <= max_rows."""
    if min(Nt, Nv, Lq) <= 0:
        raise ValueError(f"empty corpus or sequence: Nt={Nt} Nv={Nv} Lq={Lq}")
    if Lq > max_rows:
        raise ValueError(f"max_rows={max_rows} is below one fusion sequence (Lq={Lq})")
    if Nv * Lq <= max_rows:
        nt = max_rows // (Nv * Lq)
        return [(t0, min(nt, Nt - t0), 0, Nv) for t0 in range(0, Nt, nt)]
    per = max_rows // Lq                                   # videos of one block at most
    nv = -(-Nv // -(-Nv // per))                           # the same number of blocks per row, sized evenly
    return [(t, 1, v0, min(nv, Nv - v0)) for t in range(Nt) for v0 in range(0, Nv, nv)]


def retrieval_metrics(ranks):
    """eval_retrieval_tsv.py:79-91: the reference's dict of strings from the 1-based ground-truth ranks of the text queries -- recalls
    accumulated as 1 / n per hit and printed "%.2f" after * 100, `median` = int(np.median(ranks)) (an even count truncates the .5)"""
    ranks = [int(p) for p in ranks]
    if not ranks:
        raise ValueError("no queries")
    n = len(ranks)
    res = {"r@1": 0, "r@5": 0, "r@10": 0}
    for p in ranks:
        for k in (1, 5, 10):
            if p <= k:
                res[f"r@{k}"] += 1.0 / n
    out = {k: f"{v * 100:.2f}" for k, v in res.items()}
    out["median"] = f"{int(np.median(ranks))}"
    return out


class DownstreamMixin:
    # -------------------------------------------------------------- downstream: text-to-video retrieval
    # -------------------------------------------------------------- scaffolding shared by the downstream passes
    def _begin_pass(self, img, txt, train, dp_all):
        """new tape, DropPath draw, encoders -> (pool, Lv, X, Lq): one token pool of B clips' visual rows, then the text sequences' rows"""
        self.tape = []
        if train and dp_all is None:
            dp_all = self.sample_drop_path(img.shape[0])
        pool, Lv, _ = self.encode(img, None, txt, dp_all, train)
        X = txt.shape[1]
        return pool, Lv, X, Lv + X

    def _fuse_pairs(self, pool, key, pairs, B, mask, Lv, X, train, cls_only, vis_mask=None):
        """One fusion pass over the (clip i, text sequence j) pairs: rows gathered from the token pool, key mask = ones over the visual part
        (or clip i's row of `vis_mask`, u8 (B, Lv)) + the text's mask.  cls_only: the head reads the text [CLS] state alone, so the last
        layer runs for that query row only (`go_cross(qrow_split=(0, Lv))`).  -> dict(out = V of the full output or of the [CLS] rows,
        inn, idx, n_closures)."""
        dev = self.device
        ar_v, ar_t = np.arange(Lv), np.arange(X)
        idx_d = self._cached(key, lambda: _dev_i32(np.concatenate([np.concatenate([i * Lv + ar_v, B * Lv + j * X + ar_t]) for i, j in pairs]), dev))
        km_txt = (mask != 0).to(torch.uint8)
        tj = [j for _, j in pairs]
        if tj != list(range(km_txt.shape[0])):
            km_txt = km_txt[_h2d(torch.tensor(tj), dev)]
        if vis_mask is None:
            km_vis = torch.ones(len(pairs), Lv, dtype=torch.uint8, device=dev)
        else:
            ci = self._cached(("pair_clips",) + tuple(key), lambda: _h2d(torch.tensor([i for i, _ in pairs]), dev))
            km_vis = vis_mask.index_select(0, ci)
        km = torch.cat([km_vis, km_txt], 1).contiguous()
        ntape = len(self.tape)
        if cls_only:
            (_, out), inn, _ = self.go_cross(pool, idx_d, km, len(pairs), Lv + X, train, qrow_split=(0, Lv))
        else:
            out, inn, _ = self.go_cross(pool, idx_d, km, len(pairs), Lv + X, train)
        return dict(out=out, inn=inn, idx=idx_d, n_closures=len(self.tape) - ntape)

    def _cls_hidden(self, r_v, train):
        """first half of the reference's `fc` heads on the [CLS] states (Dropout(0.1), Linear H -> 2H, ReLU; main_retrieval.py:54-56,
        main_qaoe.py:42-47) -> state for `_cls_hidden_bwd`"""
        S = self.store
        p_fc = 0.1 if train else 0.0
        off_fc = self._next_offset(r_v.numel())
        r_vd = K.dropout(r_v, p_fc, self.seed, off_fc) if p_fc > 0 else r_v
        return dict(h=K.gemm(r_vd, S.b("fc.1.weight"), bias=S.p("fc.1.bias"), act=2), x=r_vd, p=p_fc, off=off_fc)

    def _cls_hidden_bwd(self, st, dh):
        """dh = d(loss)/d(hidden) with the ReLU mask already applied -> d(loss)/d([CLS] states); accumulates fc.1's gradients"""
        dr = self._linear_bwd(dh, st["x"], "fc.1.weight", "fc.1.bias")
        return K.dropout(dr, st["p"], self.seed, st["off"]) if st["p"] > 0 else dr

    def _finish_pass(self, fz, pool, dout):
        """backward of the fusion pass (its closures are the newest on the tape), the token pool's gradient through the gather, the encoders"""
        fz["out"].g = dout
        for _ in range(fz["n_closures"]):
            self.tape.pop()()
        dpool = torch.zeros((pool.t.shape[0], pool.t.shape[1]), device=self.device, dtype=F32)
        K.scatter_add_rows(fz["inn"].g, fz["idx"], dpool)
        pool.g = K.cast_bf16(dpool)
        while self.tape:
            self.tape.pop()()
        self._wgrad_join()

    # -------------------------------------------------------------- downstream: text-video retrieval
    def retrieval_forward_backward(self, img, txt, mask, train=True, backward=True, dp_all=None, dlogits=None):
        """VIOLET_Retrieval.forward + NormSoftmaxLoss (main_retrieval.py:63-85, agent.py:34-50): every (video i, text j) pair of the
        batch goes through the fusion encoder (B*B sequences gathered from one token pool), the `fc` head reads the text [CLS]
        state, and the loss is the symmetric cross entropy of the (B,B) score matrix / temp with the diagonal as targets.
        Returns (loss f32[1], scores (B,B) f32).  `dlogits` (B,B) f32 replaces d(loss)/d(scores / temp) in the backward (tests:
        the loss gradient itself is a difference of nearly equal terms whenever the scores are close, a poor probe of the
        backward path)."""
        cfg, S, dev = self.cfg, self.store, self.device
        B, Hd = img.shape[0], cfg["hidden"]
        pool, Lv, X, Lq = self._begin_pass(img, txt, train, dp_all)
        fz = self._fuse_pairs(pool, ("ret_idx", B, Lv, X), [(i, j) for i in range(B) for j in range(B)], B, mask, Lv, X, train, cls_only=True)   # (:76 reads [CLS] only)
        st = self._cls_hidden(fz["out"].t, train)
        inv_temp = 1.0 / cfg["temp"]
        lg = K.rowdot(st["h"], S.p("fc.3.weight", (2 * Hd,)), S.p("fc.3.bias"), inv_temp).view(B, B)
        tgt = torch.arange(B, dtype=torch.int64, device=dev)
        loss = torch.zeros(1, device=dev, dtype=F32)
        K.cross_entropy(lg.contiguous(), B, tgt, loss, want_grad=False)                              # -mean diag log_softmax over rows
        K.cross_entropy(lg.t().contiguous(), B, tgt, loss, want_grad=False)                          # ... and over columns
        scores = lg * cfg["temp"]
        if not backward:
            self.tape = []
            return loss, scores
        # d(loss)/d(logits) of the (B,B) matrix in f32: the useful part of this gradient is what is left after the rows / columns
        # cancel, a bf16-rounded softmax would bury it (tiny matrix: plumbing)
        eye = torch.eye(B, device=dev, dtype=F32)
        dlg = ((torch.softmax(lg, 1) - eye) / B + (torch.softmax(lg, 0) - eye) / B).reshape(-1).contiguous()
        if dlogits is not None:
            dlg = dlogits.to(dev, F32).reshape(-1).contiguous()
        dh = K.rowdot_bwd(st["h"], S.p("fc.3.weight", (2 * Hd,)), dlg, inv_temp, S.g("fc.3.weight", (2 * Hd,)), S.g("fc.3.bias"), relu_mask=True)
        self._finish_pass(fz, pool, self._cls_hidden_bwd(st, dh))
        return loss, scores

    # -------------------------------------------------------------- downstream: full-corpus retrieval evaluation (eval_retrieval_tsv.py)
    @torch.no_grad()
    def retrieval_encode_bank(self, img, txt, mask):
        """VIOLET_RetrievalEval.forward(typ='feat') (eval_retrieval.py:100-110) in eval mode, nothing kept on a tape: img f32 (B, Clips, T,
        3, H, W), txt / mask (B, X) -> (video rows bf16 (B, Lv, H) = the mean over the clips of EncVideo (f32 sums), text rows bf16
        (B, X, H), text key mask u8 (B, X))"""
        dev, Hd = self.device, self.cfg["hidden"]
        B, Cl = img.shape[0], img.shape[1]
        X = txt.shape[1]
        saved, self.tape = self.tape, NoTape()
        try:
            pool, Lv, _ = self.encode(img.reshape(B * Cl, *img.shape[2:]).to(dev, F32).contiguous(), None, txt.to(dev).contiguous(), None, False)
        finally:
            self.tape = saved
        vid = K.clip_mean(pool.t[:B * Cl * Lv], B, Cl, Lv).view(B, Lv, Hd)
        return vid, pool.t[B * Cl * Lv:].view(B, X, Hd), (mask.to(dev) != 0).to(torch.uint8)

    def _retrieval_logits(self, xv, keymask, nseq, Lq, Lv, out=None):
        """fusion encoder (last layer for the text [CLS] row only) + `fc` on assembled sequences -> fc logits f32 [nseq] (into `out`)"""
        Hd = self.cfg["hidden"]
        _, r = self.go_layers(xv, keymask, nseq, Lq, False, qrow_split=(0, Lv))
        st = self._cls_hidden(r.t, False)
        return K.rowdot(st["h"], self.store.p("fc.3.weight", (2 * Hd,)), self.store.p("fc.3.bias"), 1.0, out=out)

    @torch.no_grad()
    def retrieval_cross(self, feat_img, mask_img, feat_txt, mask_txt):
        """VIOLET_RetrievalEval.forward(typ='cross') (eval_retrieval.py:112-115) on B aligned (video, text) pairs -> fc logits f32 [B]"""
        dev, Hd = self.device, self.cfg["hidden"]
        B, Lv, X = feat_img.shape[0], feat_img.shape[1], feat_txt.shape[1]
        seq = torch.cat([feat_img.to(dev, BF16), feat_txt.to(dev, BF16)], 1).reshape(B * (Lv + X), Hd).contiguous()
        km = torch.cat([mask_img.to(dev) != 0, mask_txt.to(dev) != 0], 1).to(torch.uint8).contiguous()
        saved, self.tape = self.tape, NoTape()
        try:
            return self._retrieval_logits(V(seq), km, B, Lv + X, Lv)
        finally:
            self.tape = saved

    @torch.no_grad()
    def retrieval_corpus_scores(self, vid_bank, txt_bank, txt_mask, gt, max_rows=RETRIEVAL_MAX_ROWS):
        """Every (text, video) pair of the corpus through the fusion encoder and `fc` (eval_retrieval_tsv.py:60-77), block by block on
        the device: vid_bank bf16 (Nv, Lv, H), txt_bank bf16 (Nt, X, H), txt_mask (Nt, X), gt = bank index of each text's video.
        A block (plan_retrieval_blocks) is assembled from the banks by one kernel, runs the layers in their inference form (no tape,
        no GELU' codes, the last layer on the [CLS] row only) and writes its logits into its run of the score matrix.  Then one launch
        takes the sigmoid in place and ranks each text's video.  -> (scores f32 (Nt, Nv) on the device, ranks int32 [Nt] on the host)"""
        dev, Hd = self.device, self.cfg["hidden"]
        Nv, Lv, _ = vid_bank.shape
        Nt, X, _ = txt_bank.shape
        Lq = Lv + X
        blocks = plan_retrieval_blocks(Nt, Nv, Lq, max_rows)
        vid_bank, txt_bank = vid_bank.to(dev, BF16).contiguous(), txt_bank.to(dev, BF16).contiguous()
        txt_mask = (txt_mask.to(dev) != 0).to(torch.uint8).contiguous()
        gt_d = torch.as_tensor(np.asarray(gt, dtype=np.int32)).to(dev)
        if gt_d.numel() != Nt:
            raise ValueError(f"gt holds {gt_d.numel()} entries for {Nt} texts")
        Pmax = max(nt * nv for _, nt, _, nv in blocks)
        seq_buf = torch.empty((Pmax * Lq, Hd), device=dev, dtype=BF16)
        km_buf = torch.empty((Pmax, Lq), device=dev, dtype=torch.uint8)
        scores = torch.empty((Nt, Nv), device=dev, dtype=F32)
        flat = scores.view(-1)
        saved, self.tape = self.tape, NoTape()
        try:
            for t0, nt, v0, nv in blocks:
                P = nt * nv
                seq, km = seq_buf[:P * Lq], km_buf[:P]
                K.retrieval_assemble(vid_bank, txt_bank, txt_mask, t0, nt, v0, nv, seq, km)
                o = t0 * Nv + v0
                self._retrieval_logits(V(seq), km, P, Lq, Lv, out=flat[o:o + P])
        finally:
            self.tape = saved
        ranks = K.retrieval_rank(scores, gt_d)
        return scores, ranks.cpu()

    # -------------------------------------------------------------- downstream: open-ended video QA
    def qaoe_forward_backward(self, img, txt, mask, ans, train=True, backward=True, dp_all=None):
        """VIOLET_QAOE.forward + CrossEntropyLoss(ignore_index=-1) (main_qaoe.py:49-58,72-76, agent.py:57): one (video, question)
        fusion pass, `fc` (Dropout, Linear, ReLU, Linear -> answer vocabulary) on the text [CLS] state.  Returns (loss f32[1],
        logits (B, size_vocab) f32)."""
        cfg, S, dev = self.cfg, self.store, self.device
        B, Hd, NV = img.shape[0], cfg["hidden"], int(cfg["size_vocab"])
        pool, Lv, X, Lq = self._begin_pass(img, txt, train, dp_all)
        fz = self._fuse_pairs(pool, ("qa_idx", B, Lv, X), [(i, i) for i in range(B)], B, mask, Lv, X, train, cls_only=True)
        st = self._cls_hidden(fz["out"].t, train)
        h_v = st["h"]
        NVp = -(-NV // 8) * 8
        logits = torch.zeros((B, NVp), device=dev, dtype=F32)
        K.gemm(h_v, S.b("fc.3.weight"), N=-(-NV // 4) * 4, bias=S.p("fc.3.bias"), out=logits)
        loss = torch.zeros(1, device=dev, dtype=F32)
        dlog = K.cross_entropy(logits, NV, ans.to(dev).reshape(-1).contiguous(), loss, want_grad=backward, ld_d=NVp)
        if not backward:
            self.tape = []
            return loss, logits[:, :NV]
        K.colsum(dlog, S.g("fc.3.bias"), accumulate=True, M=B, N=NVp)
        K.gemm(dlog, h_v, a_kmajor=False, b_kmajor=False, M=NV, N=2 * Hd, K=B, out=S.g("fc.3.weight"), accumulate=True)
        dh = K.gemm(dlog, S.b("fc.3.weight"), b_kmajor=False, M=B, N=2 * Hd, K=NV, act=4, aux=h_v)            # ReLU' folded in
        self._finish_pass(fz, pool, self._cls_hidden_bwd(st, dh))
        return loss, logits[:, :NV]

    # -------------------------------------------------------------- downstream: multiple-choice video QA, MLM-head form
    def qamc_mlm_forward_backward(self, img, txt, mask, mask_ans, train=True, backward=True, dp_all=None):
        """VIOLET_QAMC_MLM_Head.forward + Agent_QAMC_MLM_Head.step (main_qamc_tsv_mlm_head.py:76-109): txt / mask / mask_ans are
        (B, O, X) -- one "question + option_o + [MASK]" sequence per option, labelled true / false token id at the [MASK] position
        and -1 elsewhere.  The clip's video tokens are shared by its O sequences (B*O sequences gathered from one token pool, as the
        retrieval head's pairs), the shared MLM head (`fc_mtm`) reads every text position, cross entropy with ignore_index -1.
        Returns (loss f32[1], logits (B*O*X, vocab) f32 view).  Task token / prompt (`enable_task_token`, `enable_prompt`) are off."""
        cfg, dev = self.cfg, self.device
        B, O, Vv = img.shape[0], int(txt.shape[1]), cfg["vocab"]
        n_seq = B * O
        txt2, mask2 = txt.reshape(n_seq, -1).contiguous(), mask.reshape(n_seq, -1).contiguous()
        pool, Lv, X, Lq = self._begin_pass(img, txt2, train, dp_all)          # pool rows: B*Lv visual, then (B*O)*X text
        fz = self._fuse_pairs(pool, ("qamc_idx", B, O, Lv, X), [(s_ // O, s_) for s_ in range(n_seq)], B, mask2, Lv, X, train, cls_only=False)
        txt_rows = self._cached(("qamc_txt_rows", n_seq, Lv, X), lambda: _dev_i32(np.concatenate([i * Lq + Lv + np.arange(X) for i in range(n_seq)]), dev))
        nr = n_seq * X
        loss = torch.zeros(1, device=dev, dtype=F32)
        hd = self._mlm_head_fwd(K.gather_rows(fz["out"].t, txt_rows, nr), nr, mask_ans.to(dev).reshape(-1).contiguous(), loss, backward)
        lg_ = hd["logits"]
        if not backward:
            self.tape = []
            return loss, lg_[:, :Vv]
        dtxt = self._mlm_head_bwd(hd)
        inv = self._cached(("qamc_inv", n_seq, Lq, Lv, X), lambda: self._inverse_rows(n_seq * Lq, [txt_rows]))
        self._finish_pass(fz, pool, K.gather_rows(dtxt, inv, n_seq * Lq))
        return loss, lg_[:, :Vv]

    # -------------------------------------------------------------- downstream: multiple-choice video QA, fc-head form
    def _select_video_tokens(self, vis, B, Lv, n, train, noise=None):
        """VIOLET_QAMC.select_vid_token (main_qamc.py:66-83) on the B clips' visual rows vis bf16 [B*Lv, H]: the two bias-free projections
        (vid_query, vid_key), then vmvm_video_token_select with vid_dropout (0.1, train only) and the gumbel noise (drawn in eval too, as
        the reference does; `noise` f32 (B, n, Lv) replaces the draw).  The reference's mask_img is all ones on this video path, so no
        visual mask is passed (NULL = every token live).  -> u8 (B, Lv) context mask.  q / k / idx / sel stay in `self.qamc_select`
        until the next pass (tests read them).  No backward: the hard `> 0` passes no gradient to vid_key / vid_query."""
        S, dev = self.store, self.device
        q = K.gemm(vis, S.b("vid_query.weight"))
        k = K.gemm(vis, S.b("vid_key.weight"))
        p = 0.1 if train else 0.0
        off_d = self._next_offset(B * n * Lv) if p > 0 else 0
        off_n = self._next_offset(B * n * Lv) if noise is None else 0
        if noise is not None:
            noise = noise.to(dev, F32).contiguous()
        idx, sel = K.video_token_select(q, k, B, Lv, n, vis_mask=None, noise=noise, dropout_p=p, seed_drop=self.seed, off_drop=off_d,
                                        seed_noise=self.seed, off_noise=off_n)
        self.qamc_select = dict(q=q, k=k, idx=idx, sel=sel)
        return sel

    def qamc_forward_backward(self, img, txt, mask, ans, train=True, backward=True, dp_all=None, noise=None, dlogits=None):
        """VIOLET_QAMC.forward + Agent_QAMC.step (main_qamc.py:85-98,142-155): txt / mask (B, O, X) = one sequence per option, ans (B,)
        the true option.  The B clips and the B*O option texts are encoded once; with num_video_tokens != -1 the clips' visual rows go
        through the token selection first and its mask becomes the visual part of the key mask.  The clip's video tokens are shared by
        its O sequences (B*O pairs gathered from one token pool), the last fusion layer runs for the text [CLS] row only, `fc` scores
        each option there, cross entropy over the O options.  Returns (loss f32[1], logits (B, O) f32) and, with the selection on, its
        context mask u8 (B, Lv) as a third element.  `dlogits` (B, O) f32 replaces d(loss)/d(logits) in the backward (tests: as
        retrieval_forward_backward's, a probe of the backward path that does not cancel across the options)."""
        cfg, S, dev = self.cfg, self.store, self.device
        B, O, Hd = img.shape[0], int(txt.shape[1]), cfg["hidden"]
        n_seq = B * O
        txt2, mask2 = txt.reshape(n_seq, -1).contiguous(), mask.reshape(n_seq, -1).contiguous()
        pool, Lv, X, Lq = self._begin_pass(img, txt2, train, dp_all)          # pool rows: B*Lv visual, then (B*O)*X text
        ntok = int(cfg.get("num_video_tokens", -1))
        sel = self._select_video_tokens(pool.t[:B * Lv], B, Lv, ntok, train, noise) if ntok != -1 else None
        fz = self._fuse_pairs(pool, ("qamc_fc_idx", B, O, Lv, X), [(s_ // O, s_) for s_ in range(n_seq)], B, mask2, Lv, X, train,
                              cls_only=True, vis_mask=sel)
        st = self._cls_hidden(fz["out"].t, train)
        logits = K.rowdot(st["h"], S.p("fc.3.weight", (2 * Hd,)), S.p("fc.3.bias"), 1.0).view(B, O)
        loss = torch.zeros(1, device=dev, dtype=F32)
        tgt = ans.to(dev, torch.int64).reshape(-1).contiguous()
        K.cross_entropy(logits, O, tgt, loss, want_grad=False)
        ret = (loss, logits) if sel is None else (loss, logits, sel)
        if not backward:
            self.tape = []
            return ret
        # d(loss)/d(logits) in f32 (tiny (B, O) matrix: plumbing).  A clip's O entries sum to zero and its O sequences share the video
        # rows: a bf16-rounded row leaves a residual that multiplies the options' common gradient and buries the signal (as for VTM)
        dlg = ((torch.softmax(logits, 1) - torch.nn.functional.one_hot(tgt, O).to(F32)) / B).reshape(-1).contiguous()
        if dlogits is not None:
            dlg = dlogits.to(dev, F32).reshape(-1).contiguous()
        dh = K.rowdot_bwd(st["h"], S.p("fc.3.weight", (2 * Hd,)), dlg, 1.0, S.g("fc.3.weight", (2 * Hd,)), S.g("fc.3.bias"), relu_mask=True)
        self._finish_pass(fz, pool, self._cls_hidden_bwd(st, dh))
        return ret
