"""Host logic of the full-corpus retrieval evaluation (eval_retrieval_tsv.py:53-91): the metric strings, the bank rules and the block
planner of the device pair loop.  No GPU."""
import numpy as np
import pytest

from pytorch_empirical_mvm_amd.downstream import build_retrieval_banks
from pytorch_empirical_mvm_amd.engine_downstream import plan_retrieval_blocks, retrieval_metrics


def _reference_rule(scores_by_text, gt):
    """eval_retrieval_tsv.py:79-91 restated from scratch: stable sort by descending score, 1-based position of the ground truth,
    recalls summed as 1/n per hit, int(np.median)"""
    res = {"r@1": 0, "r@5": 0, "r@10": 0, "median": []}
    n = len(scores_by_text)
    for t, row in enumerate(scores_by_text):
        tmp = sorted([[v, s] for v, s in enumerate(row)], key=lambda d: -d[1])
        p = [d[0] for d in tmp].index(gt[t]) + 1
        if p <= 1:
            res["r@1"] += 1.0 / n
        if p <= 5:
            res["r@5"] += 1.0 / n
        if p <= 10:
            res["r@10"] += 1.0 / n
        res["median"].append(p)
    res["median"] = int(np.median(res["median"]))
    return {k: f"{v * 100:.2f}" if k != "median" else f"{v}" for k, v in res.items()}


def _ranks(scores_by_text, gt):
    """the kernel's counting rule: 1 + #{s > s_gt} + #{v < gt : s == s_gt}"""
    out = []
    for t, row in enumerate(scores_by_text):
        row = np.asarray(row)
        g = gt[t]
        out.append(1 + int((row > row[g]).sum()) + int((row[:g] == row[g]).sum()))
    return out


@pytest.mark.parametrize("nt", [7, 8, 23, 30])                # odd and even query counts: the median truncates .5
def test_metrics_match_the_reference_rule(nt):
    rng = np.random.default_rng(nt)
    nv = 17
    scores = rng.integers(0, 6, size=(nt, nv)).astype(np.float32) / 5.0      # many exact ties
    scores[:, 3] = 1.0                                                         # a saturated column
    gt = rng.integers(0, nv, size=nt)
    want = _reference_rule(scores.tolist(), gt)
    ranks = _ranks(scores, gt)
    assert retrieval_metrics(ranks) == want
    assert list(retrieval_metrics(ranks)) == ["r@1", "r@5", "r@10", "median"]


def test_median_truncates_an_even_count():
    assert retrieval_metrics([1, 2])["median"] == "1"             # np.median = 1.5
    assert retrieval_metrics([1, 2, 4])["median"] == "2"
    assert retrieval_metrics([3, 4, 10, 11]) == {"r@1": "0.00", "r@5": "50.00", "r@10": "75.00", "median": "7"}


def test_banks_keep_the_first_video_in_order_of_appearance():
    tids = [10, 11, 12, 13, 14, 15]
    vids = ["b", "a", "b", "c", "a", "d"]
    vid_ids, txt_ids, vid_item, tid_item = build_retrieval_banks(tids, vids)
    assert vid_ids == ["b", "a", "c", "d"]
    assert vid_item == [0, 1, 3, 5]
    assert txt_ids == tids and tid_item == list(range(6))
    # a repeated text id keeps its first position and takes the last occurrence's features (dict assignment)
    vid_ids, txt_ids, vid_item, tid_item = build_retrieval_banks([5, 6, 5], ["x", "y", "x"])
    assert vid_ids == ["x", "y"] and vid_item == [0, 1]
    assert txt_ids == [5, 6] and tid_item == [2, 1]


def _check_plan(Nt, Nv, Lq, max_rows):
    blocks = plan_retrieval_blocks(Nt, Nv, Lq, max_rows)
    seen = np.zeros((Nt, Nv), dtype=np.int64)
    flat_covered = np.zeros(Nt * Nv, dtype=np.int64)
    for t0, nt, v0, nv in blocks:
        assert nt >= 1 and nv >= 1 and nt * nv * Lq <= max_rows
        assert nv == Nv or nt == 1                                # contiguous run of the row-major matrix
        seen[t0:t0 + nt, v0:v0 + nv] += 1
        # pair p = t * nv + v of the block lands at flat index (t0 + t) * Nv + v0 + v = t0 * Nv + v0 + p
        p = np.arange(nt * nv)
        flat = (t0 + p // nv) * Nv + v0 + p % nv
        assert np.array_equal(flat, t0 * Nv + v0 + p)
        flat_covered[flat] += 1
    assert (seen == 1).all() and (flat_covered == 1).all()
    return blocks


@pytest.mark.parametrize("Nt,Nv,Lq,max_rows", [(7, 5, 11, 5 * 11 * 2), (7, 5, 11, 5 * 11 * 3 - 1), (7, 5, 11, 3 * 11), (7, 5, 11, 11),
                                               (1000, 1000, 275, 1 << 18), (3, 1, 9, 9), (13, 101, 40, 1 << 12)])
def test_block_plan_covers_every_pair_once(Nt, Nv, Lq, max_rows):
    blocks = _check_plan(Nt, Nv, Lq, max_rows)
    if Nv * Lq <= max_rows:
        assert all(nv == Nv for _, _, _, nv in blocks)
    else:
        assert all(nt == 1 for _, nt, _, _ in blocks)


def test_block_plan_both_kinds_and_balance():
    assert plan_retrieval_blocks(7, 5, 11, 110) == [(0, 2, 0, 5), (2, 2, 0, 5), (4, 2, 0, 5), (6, 1, 0, 5)]
    assert plan_retrieval_blocks(2, 5, 11, 33) == [(0, 1, 0, 3), (0, 1, 3, 2), (1, 1, 0, 3), (1, 1, 3, 2)]
    b = plan_retrieval_blocks(1000, 1000, 275, 1 << 18)                        # the MSRVTT shape: two even halves per text
    assert len(b) == 2000 and {nv for *_, nv in b} == {500}
    with pytest.raises(ValueError):
        plan_retrieval_blocks(2, 2, 300, 299)
