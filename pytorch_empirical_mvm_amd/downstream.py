"""Downstream fine-tuning heads on the accelerated encoders.
* Text-to-video retrieval: `VIOLET_Retrieval` / `Agent_Retrieval` (main_retrieval.py:56-110, NormSoftmaxLoss agent.py:34-50) -- the
  batch's B x B (video, text) pairs are B*B gathered sequences of one fusion pass.
* Full-corpus text-to-video retrieval evaluation: `VIOLET_RetrievalEval` (eval_retrieval.py:100-115, eval_retrieval_tsv.py:43-91) --
  banks of clip-averaged video features and text features, every (text, video) pair of the corpus through the fusion encoder on the
  device, R@1/5/10 and the median rank.
* Open-ended video QA: `VIOLET_QAOE` / `Agent_QAOE` (main_qaoe.py:42-90) -- one (video, question) pass, classification over the
  answer vocabulary on the text [CLS] state.
* Multiple-choice video QA, fc-head form: `VIOLET_QAMC` / `Agent_QAMC` (main_qamc.py:50-155) -- one "question + option" sequence per
  option, the clip's video tokens shared by its options, `fc` scores each option at the text [CLS] state, cross entropy over the
  options; `num_video_tokens` in {48, 96, 192} first keeps the union of that many selection heads' gumbel arg-max video tokens.
* Multiple-choice video QA, MLM-head form: `VIOLET_QAMC_MLM_Head` / `Agent_QAMC_MLM_Head` (main_qamc_tsv_mlm_head.py:61-123) -- one
  "question + option + [MASK]" sequence per option, the clip's video tokens shared by its options, the pre-training MLM head
  predicts the true / false token at [MASK].
* The two single-sequence MLM-head variants: generative multiple choice `VIOLET_QAMC_MLM_Head_GEN` / `Agent_QAMC_MLM_Head_GEN`
  (main_qamc_tsv_mlm_gen_ans_idx.py:83-125: the candidate answers' token logits at [MASK]) and open-ended QA on the MLM head
  `VIOLET_QAOE_LSMDC` / `Agent_QAOE_LSMDC` = `Agent_QAOE_MLM_Head` (main_qaoe_lsmdc_fib.py:55-115, main_qaoe_tsv_mlm_head.py:101-130:
  top-1 / top-5 accuracy).
Same encoders, token pool and fusion kernels as pre-training; checkpoints interchange through the shared key names."""
import math

import torch

from . import config as CFG
from .agent import Agent_Pretrain
from .engine_downstream import RETRIEVAL_MAX_ROWS, retrieval_metrics
from .model import VIOLET_Pretrain


class VIOLET_Retrieval(VIOLET_Pretrain):
    """VIOLET_Base + `fc` (Dropout, Linear(768, 1536), ReLU, Linear(1536, 1)); checkpoint keys enc_img.* / enc_txt.* / trsfr.* / fc.*"""

    def __init__(self, args, tokzr=None, device="cuda"):
        args = CFG.Args(dict(args))
        args.update(task="retrieval", mvm_target=[])
        super().__init__(args, tokzr, device=device)

    @torch.no_grad()
    def forward(self, img, txt, mask, vid=None):
        """-> (scores (B,B) f32 = fc output of pair (video i, text j), ans = arange(B))   (main_retrieval.py:63-85)"""
        dev = self.engine.device
        _, scores = self.engine.retrieval_forward_backward(img.to(dev, torch.float32).contiguous(), txt.to(dev).contiguous(),
                                                           mask.to(dev).contiguous(), train=self.training, backward=False)
        return scores, torch.arange(img.shape[0], device=dev)


class Agent_Retrieval(Agent_Pretrain):
    """Agent_Retrieval.step (main_retrieval.py:95-110): train -> NormSoftmaxLoss(temp) + the shared backward_step (all-reduce,
    clip, AdamW, schedule); eval -> top-1 accuracy of the row arg-max."""

    def step(self, img, txt, mask, vid=None, is_train=True):
        eng = self.engine
        dev = eng.device
        img, txt, mask = img.to(dev, torch.float32).contiguous(), txt.to(dev).contiguous(), mask.to(dev).contiguous()
        if is_train:
            loss, _ = eng.retrieval_forward_backward(img, txt, mask, train=True, backward=True)
            if self.comm is not None:
                self.comm.reduce_other()
            self.backward_step()
            self.global_step += 1
            return float(loss.item())
        _, scores = eng.retrieval_forward_backward(img, txt, mask, train=False, backward=False)
        return float((scores.argmax(1) == torch.arange(img.shape[0], device=dev)).float().mean().item())


def build_retrieval_banks(tids, vids):
    """eval_retrieval_tsv.py:53-58 over the items of the evaluation in dataset order: one video bank entry per distinct video id (the
    first occurrence wins, order of first appearance) and one text bank entry per text id (order of first appearance, the last
    occurrence's features: a dict assignment).  -> (video ids, text ids, item index of each video entry, item index of each text entry)"""
    vid_ids, vid_item, tid_pos, tid_item = [], [], {}, []
    seen = set()
    for i, (t, v) in enumerate(zip(tids, vids)):
        if v not in seen:
            seen.add(v)
            vid_ids.append(v)
            vid_item.append(i)
        if t in tid_pos:
            tid_item[tid_pos[t]] = i
        else:
            tid_pos[t] = len(tid_item)
            tid_item.append(i)
    return vid_ids, list(tid_pos), vid_item, tid_item


class VIOLET_RetrievalEval(VIOLET_Retrieval):
    """eval_retrieval.py:100-115: the retrieval model (same parameters and checkpoint keys as `VIOLET_Retrieval`) with the two inference
    forms of the reference's evaluation, always in eval mode, and `evaluate_corpus`, the loop of eval_retrieval_tsv.py:43-91 with
    the pair phase on the device.  Features are the engine's bf16 rows."""

    @torch.no_grad()
    def forward(self, typ, img=None, txt=None, mask=None, feat_img=None, mask_img=None, feat_txt=None, mask_txt=None):
        """typ 'feat': img (B, Clips, T, 3, H, W), txt / mask (B, X) -> (feat_img (B, Lv, H) = mean over the clips, mask_img (B, Lv) of
        clip 0 (ones), feat_txt (B, X, H), mask_txt).  typ 'cross': B aligned (video, text) pairs -> fc logits before the sigmoid,
        `.squeeze()`d as the reference does."""
        eng = self.engine
        if typ == "feat":
            vid, trows, _ = eng.retrieval_encode_bank(img, txt, mask)
            B, Lv = vid.shape[0], vid.shape[1]
            return vid, torch.ones(B, Lv, dtype=torch.long, device=eng.device), trows, mask.to(eng.device)
        if typ == "cross":
            return eng.retrieval_cross(feat_img, mask_img, feat_txt, mask_txt).squeeze()
        raise ValueError(f"typ must be 'feat' or 'cross', got {typ!r}")

    @torch.no_grad()
    def evaluate_corpus(self, batches, gt_txt2vid, max_rows=RETRIEVAL_MAX_ROWS):
        """eval_retrieval_tsv.py:43-91.  batches: iterable of (img (B, Clips, T, 3, H, W), txt (B, X), mask (B, X), tid (B), vid (B)) as
        the reference's loader yields them; gt_txt2vid: text id -> its video id.  The banks follow `build_retrieval_banks`; every
        (text, video) pair of the banks is scored on the device (engine.retrieval_corpus_scores).
        -> dict(metrics = {'r@1', 'r@5', 'r@10', 'median'} strings as the reference prints them, scores = sigmoid scores f32 (Nt, Nv)
        on the device, ranks = int32 [Nt], txt_ids / vid_ids = the bank orders of the rows / columns)"""
        eng = self.engine
        vrows, trows, tmask, tids, vids = [], [], [], [], []
        for img, txt, mask, tid, vid in batches:
            fv, ft, km = eng.retrieval_encode_bank(img, txt, mask)
            ft = ft.clone()                                # (a view of the batch's token pool: keep the text rows only)
            for b in range(fv.shape[0]):
                vrows.append(fv[b])
                trows.append(ft[b])
                tmask.append(km[b])
            tids += [int(t) if torch.is_tensor(t) else t for t in tid]
            vids += [v.item() if torch.is_tensor(v) else v for v in vid]
        vid_ids, txt_ids, vid_item, tid_item = build_retrieval_banks(tids, vids)
        vid_bank = torch.stack([vrows[i] for i in vid_item])
        txt_bank = torch.stack([trows[i] for i in tid_item])
        txt_mask = torch.stack([tmask[i] for i in tid_item])
        del vrows, trows, tmask
        vpos = {v: i for i, v in enumerate(vid_ids)}
        gt = [vpos[gt_txt2vid[t]] for t in txt_ids]
        scores, ranks = eng.retrieval_corpus_scores(vid_bank, txt_bank, txt_mask, gt, max_rows=max_rows)
        return dict(metrics=retrieval_metrics(ranks.tolist()), scores=scores, ranks=ranks, txt_ids=txt_ids, vid_ids=vid_ids)


class VIOLET_QAOE(VIOLET_Pretrain):
    """VIOLET_Base + `fc` (Dropout, Linear(768, 1536), ReLU, Linear(1536, size_vocab))   (main_qaoe.py:42-47)"""

    def __init__(self, args, tokzr=None, device="cuda"):
        args = CFG.Args(dict(args))
        args.update(task="qaoe", mvm_target=[])
        assert int(args.get("size_vocab", 0)) > 0, "args.size_vocab (answer vocabulary) is required"
        super().__init__(args, tokzr, device=device)

    @torch.no_grad()
    def forward(self, img, txt, mask, ans):
        dev = self.engine.device
        _, logits = self.engine.qaoe_forward_backward(img.to(dev, torch.float32).contiguous(), txt.to(dev).contiguous(), mask.to(dev).contiguous(),
                                                      ans, train=self.training, backward=False)
        return logits, ans


class Agent_QAOE(Agent_Pretrain):
    """Agent_QAOE.step (main_qaoe.py:72-90): train -> CE(ignore_index=-1) + backward_step; eval -> per-sample correctness list"""

    def step(self, img, txt, mask, ans, is_train=True):
        eng = self.engine
        dev = eng.device
        img, txt, mask = img.to(dev, torch.float32).contiguous(), txt.to(dev).contiguous(), mask.to(dev).contiguous()
        if is_train:
            loss, _ = eng.qaoe_forward_backward(img, txt, mask, ans, train=True, backward=True)
            if self.comm is not None:
                self.comm.reduce_other()
            self.backward_step()
            self.global_step += 1
            return float(loss.item())
        _, logits = eng.qaoe_forward_backward(img, txt, mask, ans, train=False, backward=False)
        return (logits.argmax(1) == ans.to(dev)).float().tolist()


class VIOLET_QAMC(VIOLET_Pretrain):
    """VIOLET_Base + `fc` (Dropout, Linear(768, 1536), ReLU, Linear(1536, 1)) (+ `vid_key` / `vid_query`, bias-free Linear(768, 768), when
    num_video_tokens != -1)   (main_qamc.py:50-64).  Checkpoint keys enc_img.* / enc_txt.* / trsfr.* / fc.* (/ vid_key.weight /
    vid_query.weight); a pre-training checkpoint loads through `load_ckpt` and leaves fc / vid_* at their initial values."""

    def __init__(self, args, tokzr=None, device="cuda"):
        args = CFG.Args(dict(args))
        args.update(task="qamc", mvm_target=[])
        args.update(CFG.qamc_options(args))
        super().__init__(args, tokzr, device=device)

    @torch.no_grad()
    def forward(self, img, txt, mask, ans):
        """img (B, T, 3, H, W), txt / mask (B, O, X), ans (B,) -> (out (B, O) f32 = fc at each option's text [CLS], ans)   (:85-98)"""
        dev = self.engine.device
        r = self.engine.qamc_forward_backward(img.to(dev, torch.float32).contiguous(), txt.to(dev).contiguous(), mask.to(dev).contiguous(),
                                              ans.to(dev), train=self.training, backward=False)
        return r[1], ans

    @torch.no_grad()
    def reinit_head(self):
        """main_qamc.py:100-103: a fresh `fc` with nn.Linear's default initialisation (weight and bias U(+-1/sqrt(fan_in)), torch's global
        generator, as the reference's module constructor draws)"""
        S = self.engine.store
        S.sync_pending()
        for name in ("fc.1.weight", "fc.1.bias", "fc.3.weight", "fc.3.bias"):
            fan_in = self.hidden_size if name.startswith("fc.1.") else 2 * self.hidden_size
            b = 1.0 / math.sqrt(fan_in)
            S.p(name).copy_(torch.empty(S.index[name][2]).uniform_(-b, b).to(S.device))
        S.refresh_shadow()


class Agent_QAMC(Agent_Pretrain):
    """Agent_QAMC (main_qamc.py:105-155).  step: train -> CrossEntropyLoss over the options + the shared backward_step (all-reduce, clip,
    AdamW, schedule); eval -> per-clip correctness of the arg-max option.  Optimizer groups (build_optimizer :111-140): the
    `vis_backbone_lr_mul` groups are the parameters named `fc.*` (NOT the Video-Swin backbone, despite the variable names), everything
    else runs at the base rate; vid_key / vid_query never get a gradient, so AdamW skips them (no update, no decay)."""

    def __init__(self, args, model):
        super().__init__(args, model)
        S = self.engine.store
        self._fc_tail = {gi: S.tail_start(gi, "fc.") for gi in (1, 3)}        # fc.* = the tail of the two non-Swin segments (asserted)
        self.log = {"ls_tr": [], "ac_vl": [], "ac_ts": []}

    def current_lrs(self):
        """the reference's four groups in its order: [fc decay, other decay, fc no-decay, other no-decay]"""
        f = CFG.lr_factor(self.sched_step, self.args.max_iter)
        fc, other = max(1e-8, self.args.lr * self.args.vis_backbone_lr_mul * f), max(1e-8, self.args.lr * f)
        return [fc, other, fc, other]

    def segment_runs(self, gi, lrs):
        """arena segment gi (0 / 2: Swin, 1 / 3: the rest, decay / no-decay) -> runs at the base rate, then fc.* at the multiplied one"""
        a, e = self.engine.store.segments[gi]
        base, fc = (lrs[1], lrs[0]) if gi < 2 else (lrs[3], lrs[2])
        t = self._fc_tail.get(gi, e)
        return [r for r in ((a, t, base), (t, e, fc)) if r[1] > r[0]]

    def step(self, img, txt, mask, ans, is_train=True):
        eng = self.engine
        dev = eng.device
        img, txt, mask = img.to(dev, torch.float32).contiguous(), txt.to(dev).contiguous(), mask.to(dev).contiguous()
        ans = ans.to(dev)
        if is_train:
            loss = eng.qamc_forward_backward(img, txt, mask, ans, train=True, backward=True)[0]
            if self.comm is not None:
                self.comm.reduce_other()
            self.backward_step()
            self.global_step += 1
            return float(loss.item())
        logits = eng.qamc_forward_backward(img, txt, mask, ans, train=False, backward=False)[1]
        return (logits.argmax(1) == ans).float().tolist()


class VIOLET_QAMC_MLM_Head(VIOLET_Pretrain):
    """VIOLET_Base + the pre-training MLM head `fc_mtm` (+ `emb_task`, unused while the task token is off); no `fc`
    (main_qamc_tsv_mlm_head.py:61-71).  A pre-training checkpoint loads through `load_ckpt` (shared key names)."""

    def __init__(self, args, tokzr=None, device="cuda"):
        args = CFG.Args(dict(args))
        args.update(task="qamc_mlm", mvm_target=[])
        if args.get("enable_task_token") or args.get("enable_prompt"):
            raise NotImplementedError("task token / prompt prefixes (model.py:219-293) are outside the accelerated path")
        super().__init__(args, tokzr, device=device)

    @torch.no_grad()
    def forward(self, batch):
        """batch: img (B,T,3,H,W), txt / mask / mask_ans (B,O,X) -> (out (B*O, X, vocab) f32, ans (B,O,X))   (:76-94)"""
        dev = self.engine.device
        txt = batch["txt"]
        B, O, X = txt.shape
        _, lg = self.engine.qamc_mlm_forward_backward(batch["img"].to(dev, torch.float32).contiguous(), txt.to(dev), batch["mask"].to(dev),
                                                      batch["mask_ans"].to(dev), train=self.training, backward=False)
        return lg.view(B * O, X, -1), batch["mask_ans"].to(dev)


class Agent_QAMC_MLM_Head(Agent_Pretrain):
    """Agent_QAMC_MLM_Head.step (main_qamc_tsv_mlm_head.py:100-123): train -> cross entropy over the text positions (ignore -1) + the
    shared backward_step; eval -> per-clip accuracy of arg-max over the options of p_true / (p_true + p_false) at [MASK]."""

    def __init__(self, args, model, true_token_id=2995, false_token_id=6270):       # bert-base-uncased ids of "true" / "false"
        super().__init__(args, model)
        self.true_token_id, self.false_token_id = int(true_token_id), int(false_token_id)

    def current_lrs(self):
        """Agent_QAMC.build_optimizer (main_qamc.py:111-140): the `vis_backbone_lr_mul` group is the parameters whose name starts with
        `fc.` -- none in the MLM-head model -- so every group runs at the base rate."""
        lr = max(1e-8, self.args.lr * CFG.lr_factor(self.sched_step, self.args.max_iter))
        return [lr, lr, lr, lr]

    def step(self, batch, is_train=True):
        eng = self.engine
        dev = eng.device
        img = batch["img"].to(dev, torch.float32).contiguous()
        txt, mask, ans = batch["txt"].to(dev), batch["mask"].to(dev), batch["mask_ans"].to(dev)
        if is_train:
            loss, _ = eng.qamc_mlm_forward_backward(img, txt, mask, ans, train=True, backward=True)
            if self.comm is not None:
                self.comm.reduce_other()
            self.backward_step()
            self.global_step += 1
            return float(loss.item())
        B, O, X = txt.shape
        _, lg = eng.qamc_mlm_forward_backward(img, txt, mask, ans, train=False, backward=False)
        lg = lg.view(B * O, X, -1)
        pt, pf = lg[:, :, self.true_token_id], lg[:, :, self.false_token_id]
        sc = pt / (pt + pf)
        m = ans.reshape(B * O, X)
        sc, am = sc[m != -1].view(B, O), m[m != -1].view(B, O)
        return (sc.argmax(-1) == (am == self.true_token_id).nonzero()[:, 1]).float().tolist()


class VIOLET_QAMC_MLM_Head_GEN(VIOLET_QAMC_MLM_Head):
    """main_qamc_tsv_mlm_gen_ans_idx.py:83-101: ONE "question + options + [MASK]" sequence per clip -- txt / mask / mask_ans (B, X) --
    through the same encoders and MLM head (the multiple-choice pass with a single option per clip)."""

    @torch.no_grad()
    def forward(self, batch):
        """-> (out (B, X, vocab) f32, ans (B, X))"""
        dev = self.engine.device
        txt = batch["txt"]
        B, X = txt.shape
        _, lg = self.engine.qamc_mlm_forward_backward(batch["img"].to(dev, torch.float32).contiguous(), txt.to(dev)[:, None], batch["mask"].to(dev)[:, None],
                                                      batch["mask_ans"].to(dev)[:, None], train=self.training, backward=False)
        return lg.view(B, X, -1), batch["mask_ans"].to(dev)


class VIOLET_QAOE_LSMDC(VIOLET_QAMC_MLM_Head_GEN):
    """main_qaoe_lsmdc_fib.py:55-84 (`size_vocab == -1`: the answer is a token of the MLM vocabulary): same forward as the generative
    multiple-choice model."""


VIOLET_QAOE_MLM_Head = VIOLET_QAOE_LSMDC            # main_qaoe_tsv_mlm_head.py builds VIOLET_QAOE_LSMDC under this task name


class _Agent_MLM_QA(Agent_QAMC_MLM_Head):
    """shared train branch: CE(ignore_index=-1) over the text positions of the single-sequence form + the shared backward_step"""

    def _fwd(self, batch, is_train):
        eng, dev = self.engine, self.engine.device
        img = batch["img"].to(dev, torch.float32).contiguous()
        txt, mask, ans = batch["txt"].to(dev), batch["mask"].to(dev), batch["mask_ans"].to(dev)
        loss, lg = eng.qamc_mlm_forward_backward(img, txt[:, None], mask[:, None], ans[:, None], train=is_train, backward=is_train)
        return loss, lg.view(txt.shape[0], txt.shape[1], -1), ans

    def _train(self, batch):
        loss, _, _ = self._fwd(batch, True)
        if self.comm is not None:
            self.comm.reduce_other()
        self.backward_step()
        self.global_step += 1
        return float(loss.item())


class Agent_QAMC_MLM_Head_GEN(_Agent_MLM_QA):
    """Agent_QAMC_MLM_Head_GEN.step (main_qamc_tsv_mlm_gen_ans_idx.py:103-125).  eval: the RAW logits of the candidate answer tokens
    `ans_tok_ids` at the clip's [MASK] position, divided by their sum, arg-max against batch["ans_idx"] -> per-clip correctness."""

    def __init__(self, args, model, ans_tok_ids):
        super().__init__(args, model)
        self.ans_tok_ids = [int(i) for i in ans_tok_ids]

    def step(self, batch, is_train=True):
        if is_train:
            return self._train(batch)
        _, out, ans = self._fwd(batch, False)
        B = ans.shape[0]
        p = out[:, :, self.ans_tok_ids][ans != -1]
        p = (p / p.sum(dim=-1).view(B, 1)).view(B, -1)
        return (p.argmax(dim=-1) == batch["ans_idx"].to(p.device)).float().tolist()


class Agent_QAOE_LSMDC(_Agent_MLM_QA):
    """Agent_QAOE_LSMDC.step / get_top_k_acc (main_qaoe_lsmdc_fib.py:86-112): train -> {'ls'}; eval -> {'ac_1', 'ac_5'} per-clip lists"""

    def step(self, batch, is_train=True):
        if is_train:
            return {"ls": self._train(batch)}
        _, out, ans = self._fwd(batch, False)
        return {"ac_1": self.get_top_k_acc(out, ans, k=1), "ac_5": self.get_top_k_acc(out, ans, k=5)}

    @staticmethod
    def get_top_k_acc(out, ans, k=5):
        """1.0 per labelled position whose label is among the k largest logits; padded with 0.0 to the batch size"""
        B = out.shape[0]
        sel = ans != -1
        ac = []
        if bool(sel.any()):
            lab = ans[sel].view(-1, 1)
            top = torch.topk(out[sel].view(lab.shape[0], -1), k=k, dim=-1).indices
            ac = (top == lab).any(dim=-1).float().tolist()
        return ac + [0.0] * (B - len(ac))


Agent_QAOE_MLM_Head = Agent_QAOE_LSMDC              # main_qaoe_tsv_mlm_head.py:101-105 adds only the optional freeze
