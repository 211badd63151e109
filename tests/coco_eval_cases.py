"""COCO box evaluation: a NumPy float64 restatement of the algorithm as plain loops (per image, per category, per area
range, per threshold, one detection and one ground truth at a time -- nothing shared with the package's vectorised
composite), and the builders of the test cases.

An image of a case is a dict: ``image_id``, ``det_scores`` f32 [n], ``det_labels`` i64 [n], ``det_boxes`` f32 [n, 4] xyxy,
``gt_boxes`` f32 [g, 4], ``gt_labels`` i64 [g], ``gt_crowd`` u8 [g], ``gt_area`` f64 [g] or None (then w * h)."""
import numpy as np
import torch

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0.0, 1e10], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, 1e10]]


def box_iou(d, g, crowd):
    d = [float(v) for v in d]
    g = [float(v) for v in g]
    iw = min(d[2], g[2]) - max(d[0], g[0])
    ih = min(d[3], g[3]) - max(d[1], g[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    d_area = (d[2] - d[0]) * (d[3] - d[1])
    union = d_area if crowd else d_area + (g[2] - g[0]) * (g[3] - g[1]) - inter
    return inter / union


def evaluate_image(img, cat, area_rng):
    """One (image, category, area range): ``None`` if the image has neither, else the sorted detection scores and the
    ``[10][D]`` matched / ignored flags, and the ground truths' ignore flags."""
    gts = [i for i in range(len(img["gt_labels"])) if int(img["gt_labels"][i]) == cat]
    dts = [i for i in range(len(img["det_labels"])) if int(img["det_labels"][i]) == cat]
    if not gts and not dts:
        return None
    gt_ignore = []
    for i in gts:
        if img["gt_area"] is not None:
            area = float(img["gt_area"][i])
        else:
            b = [float(v) for v in img["gt_boxes"][i]]
            area = (b[2] - b[0]) * (b[3] - b[1])
        gt_ignore.append(1 if (img["gt_crowd"][i] or area < area_rng[0] or area > area_rng[1]) else 0)
    gt_order = sorted(range(len(gts)), key=lambda i: gt_ignore[i])                  # stable
    gts = [gts[i] for i in gt_order]
    gt_ignore = [gt_ignore[i] for i in gt_order]
    dts = sorted(dts, key=lambda i: -float(img["det_scores"][i]))[:100]            # stable
    gt_matched = [[False] * len(gts) for _ in IOU_THRS]
    dt_matched = [[False] * len(dts) for _ in IOU_THRS]
    dt_ignore = [[False] * len(dts) for _ in IOU_THRS]
    for ti, t in enumerate(IOU_THRS):
        for di, d in enumerate(dts):
            best, m = min(t, 1 - 1e-10), -1
            for gi, g in enumerate(gts):
                crowd = bool(img["gt_crowd"][g])
                if gt_matched[ti][gi] and not crowd:
                    continue
                if m > -1 and gt_ignore[m] == 0 and gt_ignore[gi] == 1:
                    break
                iou = box_iou(img["det_boxes"][d], img["gt_boxes"][g], crowd)
                if iou < best:
                    continue
                best, m = iou, gi
            if m == -1:
                continue
            dt_ignore[ti][di] = bool(gt_ignore[m])
            dt_matched[ti][di] = True
            gt_matched[ti][m] = True
    for di, d in enumerate(dts):
        b = [float(v) for v in img["det_boxes"][d]]
        area = (b[2] - b[0]) * (b[3] - b[1])
        for ti in range(len(IOU_THRS)):
            if not dt_matched[ti][di] and (area < area_rng[0] or area > area_rng[1]):
                dt_ignore[ti][di] = True
    return {"scores": [float(img["det_scores"][d]) for d in dts], "matched": dt_matched, "ignored": dt_ignore,
            "gt_ignore": gt_ignore}


def restate(category_ids, images):
    """The whole evaluation.  Returns ``precision``, ``recall``, ``scores``, ``stats`` and, for comparing records,
    ``bits[(image id, category index, rank)] = (score, matched word, ignored word)`` and
    ``npig[(image id, category index)] = [4 counts]``."""
    cats = sorted(set(int(c) for c in category_ids))
    images = sorted(images, key=lambda im: int(im["image_id"]))
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cats), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    bits, npig_of = {}, {}
    for k, cat in enumerate(cats):
        for a, rng in enumerate(AREA_RNG):
            results = [evaluate_image(im, cat, rng) for im in images]
            for im, e in zip(images, results):
                if e is None:
                    continue
                if e["gt_ignore"]:
                    npig_of.setdefault((int(im["image_id"]), k), [0] * A)[a] = sum(1 for g in e["gt_ignore"] if g == 0)
                for rank in range(len(e["scores"])):
                    s, mw, iw = bits.get((int(im["image_id"]), k, rank), (e["scores"][rank], 0, 0))
                    for ti in range(T):
                        mw |= int(e["matched"][ti][rank]) << (a * T + ti)
                        iw |= int(e["ignored"][ti][rank]) << (a * T + ti)
                    bits[(int(im["image_id"]), k, rank)] = (s, mw, iw)
            results = [e for e in results if e is not None]
            for m, max_det in enumerate(MAX_DETS):
                if not results:
                    continue
                all_scores = np.array([s for e in results for s in e["scores"][:max_det]], dtype=np.float64)
                order = np.argsort(-all_scores, kind="mergesort")
                npig = sum(1 for e in results for g in e["gt_ignore"] if g == 0)
                if npig == 0:
                    continue
                for ti in range(T):
                    matched = [v for e in results for v in e["matched"][ti][:max_det]]
                    ignored = [v for e in results for v in e["ignored"][ti][:max_det]]
                    tp_run = fp_run = 0
                    rc, pr = [], []
                    for i in order:
                        tp_run += 1 if (matched[i] and not ignored[i]) else 0
                        fp_run += 1 if (not matched[i] and not ignored[i]) else 0
                        rc.append(tp_run / npig)
                        pr.append(tp_run / (fp_run + tp_run + np.spacing(1)))
                    recall[ti, k, a, m] = rc[-1] if rc else 0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    where = np.searchsorted(np.array(rc, dtype=np.float64), REC_THRS, side="left")
                    for ri, pi in enumerate(where):
                        precision[ti, ri, k, a, m] = pr[pi] if pi < len(pr) else 0.0
                        scores[ti, ri, k, a, m] = all_scores[order[pi]] if pi < len(pr) else 0.0

    def mean_of(values):
        values = values[values > -1]
        return float(np.mean(values)) if values.size else -1.0
    stats = [mean_of(precision[:, :, :, 0, 2]), mean_of(precision[0, :, :, 0, 2]), mean_of(precision[5, :, :, 0, 2]),
             mean_of(precision[:, :, :, 1, 2]), mean_of(precision[:, :, :, 2, 2]), mean_of(precision[:, :, :, 3, 2]),
             mean_of(recall[:, :, 0, 0]), mean_of(recall[:, :, 0, 1]), mean_of(recall[:, :, 0, 2]),
             mean_of(recall[:, :, 1, 2]), mean_of(recall[:, :, 2, 2]), mean_of(recall[:, :, 3, 2])]
    return {"precision": precision, "recall": recall, "scores": scores, "stats": np.array(stats), "bits": bits,
            "npig": npig_of}


def accumulate_rows(ranks, row_scores, matched_words, ignored_words, npig):
    """One category from its records in final order (plain lists; bit ``area * 10 + threshold``): ``precision`` and
    ``scores`` [10, 101, 4, 3], ``recall`` [10, 4, 3], as loops."""
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision, recall, scores = -np.ones((T, R, A, M)), -np.ones((T, A, M)), -np.ones((T, R, A, M))
    for a in range(A):
        if npig[a] == 0:
            continue
        for m, max_det in enumerate(MAX_DETS):
            rows = [i for i in range(len(ranks)) if ranks[i] < max_det]
            for ti in range(T):
                bit = a * T + ti
                tp_run = fp_run = 0
                rc, pr = [], []
                for i in rows:
                    matched, ignored = (matched_words[i] >> bit) & 1, (ignored_words[i] >> bit) & 1
                    tp_run += 1 if (matched and not ignored) else 0
                    fp_run += 1 if (not matched and not ignored) else 0
                    rc.append(tp_run / npig[a])
                    pr.append(tp_run / (fp_run + tp_run + np.spacing(1)))
                recall[ti, a, m] = rc[-1] if rc else 0
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                where = np.searchsorted(np.array(rc, dtype=np.float64), REC_THRS, side="left")
                for ri, pi in enumerate(where):
                    precision[ti, ri, a, m] = pr[pi] if pi < len(pr) else 0.0
                    scores[ti, ri, a, m] = row_scores[rows[pi]] if pi < len(pr) else 0.0
    return precision, recall, scores


# ---- case builders -------------------------------------------------------------------------------------------------------
def image(image_id, dets=(), gts=()):
    """``dets``: (score, label, box); ``gts``: (label, box[, crowd[, area]])."""
    gts = [tuple(g) + (0, None)[len(g) - 2:] for g in gts]
    areas = [g[3] for g in gts]
    assert all(a is None for a in areas) or all(a is not None for a in areas)
    return {"image_id": image_id,
            "det_scores": np.array([d[0] for d in dets], dtype=np.float32),
            "det_labels": np.array([d[1] for d in dets], dtype=np.int64),
            "det_boxes": np.array([d[2] for d in dets], dtype=np.float32).reshape(-1, 4),
            "gt_boxes": np.array([g[1] for g in gts], dtype=np.float32).reshape(-1, 4),
            "gt_labels": np.array([g[0] for g in gts], dtype=np.int64),
            "gt_crowd": np.array([g[2] for g in gts], dtype=np.uint8),
            "gt_area": np.array(areas, dtype=np.float64) if gts and areas[0] is not None else None}


def known_cases():
    """The cases with answers known in advance: name -> (category ids, images)."""
    unit = [0, 0, 10, 10]
    return {
        "A": ([1], [image(1, [(0.9, 1, unit)], [(1, unit)])]),
        "B": ([1], [image(1, [(0.9, 1, [20, 20, 30, 30]), (0.8, 1, unit)], [(1, unit)])]),
        "C": ([1], [image(1, [(0.9, 1, [0, 0, 100, 77])], [(1, [0, 0, 100, 100])])]),
        "D": ([1], [image(1, [(0.9, 1, [2, 2, 8, 8])], [(1, [0, 0, 10, 10], 1)])]),
        "E": ([1], [image(1, [(0.9, 1, [0, 0, 32, 32])], [(1, [0, 0, 32, 32])])]),
    }


def clear_of_thresholds(images, margin=1e-9):
    """No IoU of a same-label (detection, ground truth) pair within ``margin`` of a threshold."""
    for im in images:
        for d in range(len(im["det_labels"])):
            for g in range(len(im["gt_labels"])):
                if int(im["det_labels"][d]) != int(im["gt_labels"][g]):
                    continue
                iou = box_iou(im["det_boxes"][d], im["gt_boxes"][g], bool(im["gt_crowd"][g]))
                if np.abs(IOU_THRS - iou).min() <= margin:
                    return False
    return True


def _random_box(rng):
    side = [6, 14, 28, 40, 70, 110, 150][rng.integers(7)]
    w, h = int(side * rng.uniform(0.6, 1.4)) + 1, int(side * rng.uniform(0.6, 1.4)) + 1
    x, y = int(rng.integers(0, 200)), int(rng.integers(0, 200))
    return [x, y, x + w, y + h]


def _jitter(rng, box):
    w, h = box[2] - box[0], box[3] - box[1]
    dx = [int(rng.integers(-max(1, w // 5), max(1, w // 5) + 1)) for _ in range(2)]
    dy = [int(rng.integers(-max(1, h // 5), max(1, h // 5) + 1)) for _ in range(2)]
    x1, y1 = box[0] + dx[0], box[1] + dy[0]
    return [x1, y1, max(x1 + 1, box[2] + dx[1]), max(y1 + 1, box[3] + dy[1])]


CATEGORY_IDS = [11, 2, 5]          # non-contiguous, given unsorted
SCORES = [0.9375, 0.875, 0.75, 0.625, 0.5, 0.5, 0.375, 0.25, 0.125]        # few values: ties within and across images


def random_scene(seed=0):
    """4 images (ids out of order): one without detections, one without ground truths, a detection label outside the
    categories, crowds over several detections, duplicated ground truths, tied scores.  Boxes on an integer grid."""
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        images = []
        for image_id, n_gt, n_det in ((42, 12, 20), (7, 9, 0), (19, 0, 14), (3, 11, 20)):
            gts, dets = [], []
            for i in range(n_gt):
                label = CATEGORY_IDS[rng.integers(3)]
                if gts and i % 5 == 4:
                    gts.append(gts[rng.integers(len(gts))])                 # a duplicate: the equal-IoU rule
                    continue
                box = _random_box(rng)
                crowd = 1 if i % 6 == 5 else 0
                if crowd:
                    box = [box[0], box[1], box[0] + 160, box[1] + 120]      # a crowd region over several detections
                gts.append((label, box, crowd))
            for i in range(n_det):
                score = SCORES[rng.integers(len(SCORES))]
                if i == 3:
                    dets.append((score, 7, _random_box(rng)))                # 7 is no category
                elif gts and rng.uniform() < 0.7:
                    g = gts[rng.integers(len(gts))]
                    if g[2]:
                        x, y = g[1][0] + int(rng.integers(0, 100)), g[1][1] + int(rng.integers(0, 80))
                        dets.append((score, g[0], [x, y, x + int(rng.integers(5, 60)), y + int(rng.integers(5, 40))]))
                    else:
                        dets.append((score, g[0], _jitter(rng, g[1]) if rng.uniform() < 0.8 else list(g[1])))
                else:
                    dets.append((score, CATEGORY_IDS[rng.integers(3)], _random_box(rng)))
            images.append(image(image_id, dets, gts))
        if clear_of_thresholds(images):
            break
    assert clear_of_thresholds(images), "no IoU may lie within 1e-9 of a threshold"
    return CATEGORY_IDS, images


def cap_scene():
    """130 detections of one category in one image (the cap at 100, ranks for maxDet 1 / 10), a second image beside it."""
    rng = np.random.default_rng(77)
    gts = [(5, [10 + 40 * i, 10, 40 + 40 * i, 50]) for i in range(4)] + [(2, [5, 100, 60, 170])]
    dets = []
    for i in range(130):
        g = gts[i % 4]
        box = _jitter(rng, g[1]) if i % 3 else _random_box(rng)
        dets.append((float(np.float32(0.05 + 0.9 * rng.uniform())) if i % 7 else 0.5, 5, box))
    dets += [(0.75, 2, [5, 100, 60, 168]), (0.5, 2, [0, 0, 9, 9])]
    images = [image(8, dets, gts), image(2, [(0.5, 5, [12, 10, 40, 52])], [(5, [10, 10, 40, 50])])]
    assert clear_of_thresholds(images), "no IoU may lie within 1e-9 of a threshold"
    return CATEGORY_IDS, images


# ---- to the evaluator's inputs ---------------------------------------------------------------------------------------------
def as_update_args(images, device="cpu"):
    """(``PostProcess``-style list of dicts, targets) of ``images`` on ``device``."""
    detections, targets = [], []
    for im in images:
        detections.append({"scores": torch.from_numpy(im["det_scores"]).to(device),
                           "labels": torch.from_numpy(im["det_labels"]).to(device),
                           "boxes": torch.from_numpy(im["det_boxes"]).to(device)})
        target = {"image_id": int(im["image_id"]), "boxes": torch.from_numpy(im["gt_boxes"]).to(device),
                  "labels": torch.from_numpy(im["gt_labels"]).to(device),
                  "iscrowd": torch.from_numpy(im["gt_crowd"]).to(device)}
        if im["gt_area"] is not None:
            target["area"] = torch.from_numpy(im["gt_area"]).to(device)
        targets.append(target)
    return detections, targets


def record_bits(det_records):
    """Detection records [N, 5] -> {(image id, category index, rank): (score, matched word, ignored word)}."""
    out = {}
    rows = det_records.cpu()
    scores = rows[:, 2].contiguous().view(torch.float64).tolist()
    for row, score in zip(rows.tolist(), scores):
        out[(row[0], row[1] & 0xFFFFFFFF, row[1] >> 32)] = (score, row[3], row[4])
    return out


def record_npig(gt_records):
    return {(row[0], row[1]): row[2:6] for row in gt_records.cpu().tolist()}
