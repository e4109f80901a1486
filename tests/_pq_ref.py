"""The reference of the panoptic-quality tests (csrc/panoptic_quality.hip, ops.pq_image / pq_reduce, CocoPanopticMetric),
restated in numpy from the semantics of mmdet's pq_compute_single_core and _parse_predictions and of panopticapi's
PQStat.pq_average -- not copied from either.  Two forms that must agree (tests/test_pq_cpu.py asserts it on every generated
input): `image_loop`, the dict-and-loop procedure over np.unique keys, and `image_arrays`, bincount over dense slots.

An image's result: dict(stat={category id: [tp, fp, fn, iou_sum]} over `categories`, segments=[(id, category id, area)] in
ascending id).  Doubles are Python floats: iou = inter / union is one IEEE division, sums run in ascending gt id."""
import numpy as np

OFFSET = 1000                           # INSTANCE_OFFSET
VOID = 0


def rgb2id(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


def id2rgb(ids):
    ids = np.asarray(ids).astype(np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536 % 256], axis=-1).astype(np.uint8)


def void_mapped(pan, num_classes, ignore_index=None):
    """the prediction as the evaluation reads it: void pixels are 0"""
    ignore_index = num_classes if ignore_index is None else ignore_index
    pan = np.asarray(pan).astype(np.int64).copy()
    lab = pan % OFFSET
    pan[(lab == num_classes) | (lab == ignore_index)] = VOID
    return pan


def _pred_segments(pan0, label2cat, categories):
    """[(id, category, area)] of the distinct non-void ids, ascending"""
    out = []
    ids, counts = np.unique(pan0, return_counts=True)
    for i, n in zip(ids.tolist(), counts.tolist()):
        if i == VOID:
            continue
        lab = i % OFFSET
        cat = label2cat[lab] if label2cat is not None else lab
        if cat not in categories:
            raise KeyError(f'segment {i} has unknown category_id {cat}')
        out.append((i, cat, n))
    return out


def _gt_with_areas(gt, gt_segments):
    return [dict(s, area=int((gt == s['id']).sum()) if s.get('area') is None else int(s['area'])) for s in gt_segments]


def image_loop(pan, gt, gt_segments, categories, num_classes, ignore_index=None, label2cat=None):
    """the procedure, step by step with dicts"""
    categories = list(categories)
    gt = np.asarray(gt).astype(np.int64)
    pan0 = void_mapped(pan, num_classes, ignore_index)
    segments = _pred_segments(pan0, label2cat, categories)
    pred = {i: dict(category_id=c, area=a) for i, c, a in segments}
    gts = {s['id']: s for s in _gt_with_areas(gt, gt_segments)}
    assert len(gts) == len(gt_segments), 'duplicate gt ids'
    big = 1 << 32
    keys, counts = np.unique(gt * big + pan0, return_counts=True)
    conf = {(k // big, k % big): n for k, n in zip(keys.tolist(), counts.tolist())}
    stat = {}

    def at(cat):
        return stat.setdefault(cat, [0, 0, 0, 0.0])

    g_matched, p_matched = set(), set()
    for (g, p), inter in conf.items():                    # ascending (gt id, pred id): np.unique sorts the keys
        if g not in gts or p not in pred or gts[g]['iscrowd'] == 1 or gts[g]['category_id'] != pred[p]['category_id']:
            continue
        union = pred[p]['area'] + gts[g]['area'] - inter - conf.get((VOID, p), 0)
        iou = inter / union
        if iou > 0.5:
            at(gts[g]['category_id'])[0] += 1
            at(gts[g]['category_id'])[3] += iou
            g_matched.add(g)
            p_matched.add(p)
    crowd_of = {}
    for g, info in gts.items():                           # JSON order: a later crowd segment replaces an earlier one
        if g in g_matched:
            continue
        if info['iscrowd'] == 1:
            crowd_of[info['category_id']] = g
            continue
        at(info['category_id'])[2] += 1
    for p, info in pred.items():
        if p in p_matched:
            continue
        inter = conf.get((VOID, p), 0)
        if info['category_id'] in crowd_of:
            inter += conf.get((crowd_of[info['category_id']], p), 0)
        if inter / info['area'] > 0.5:
            continue
        at(info['category_id'])[1] += 1
    return dict(stat={c: stat.get(c, [0, 0, 0, 0.0]) for c in categories}, segments=segments)


def image_arrays(pan, gt, gt_segments, categories, num_classes, ignore_index=None, label2cat=None):
    """the same result from one bincount over dense (gt slot, pred slot) pairs"""
    categories = list(categories)
    gt = np.asarray(gt).astype(np.int64).ravel()
    pan0 = void_mapped(pan, num_classes, ignore_index).ravel()
    order = sorted(range(len(gt_segments)), key=lambda k: gt_segments[k]['id'])
    gid = np.array([gt_segments[k]['id'] for k in order], dtype=np.int64)
    G = len(order)
    pid = np.unique(pan0)
    pid = pid[pid != VOID]
    P = len(pid)
    # rows: 0 VOID, 1 + slot, G + 1 unlisted; columns: 0 void, 1 + slot
    gs = np.full(gt.shape, G + 1, dtype=np.int64)
    gs[gt == VOID] = 0
    if G:
        pos = np.minimum(np.searchsorted(gid, gt), G - 1)
        hit = (gid[pos] == gt) & (gt != VOID)
        gs[hit] = pos[hit] + 1
    ps = np.where(pan0 == VOID, 0, np.searchsorted(pid, pan0) + 1) if P else np.zeros(pan0.shape, dtype=np.int64)
    conf = np.bincount(gs * (P + 1) + ps, minlength=(G + 2) * (P + 1)).reshape(G + 2, P + 1)
    p_area = conf.sum(axis=0)
    p_cat = []
    for i in pid.tolist():
        cat = label2cat[i % OFFSET] if label2cat is not None else i % OFFSET
        if cat not in categories:
            raise KeyError(f'segment {i} has unknown category_id {cat}')
        p_cat.append(cat)
    g_area = [int(conf[j + 1].sum()) if gt_segments[k].get('area') is None else int(gt_segments[k]['area'])
              for j, k in enumerate(order)]
    g_cat = [gt_segments[k]['category_id'] for k in order]
    g_crowd = [gt_segments[k]['iscrowd'] == 1 for k in order]
    stat = {c: [0, 0, 0, 0.0] for c in set(categories) | set(g_cat)}
    p_matched = np.zeros(P + 1, dtype=bool)
    for j in range(G):                                    # ascending gt id
        if g_crowd[j]:
            continue
        found = False
        for p in np.nonzero(conf[j + 1, 1:])[0] + 1:
            if p_cat[p - 1] != g_cat[j]:
                continue
            inter = int(conf[j + 1, p])
            iou = inter / (int(p_area[p]) + g_area[j] - inter - int(conf[0, p]))
            if iou > 0.5:
                stat[g_cat[j]][0] += 1
                stat[g_cat[j]][3] += iou
                p_matched[p] = found = True
        if not found:
            stat[g_cat[j]][2] += 1
    slot_of = {int(i): j for j, i in enumerate(gid.tolist())}
    crowd_of = {}
    for s in gt_segments:
        if s['iscrowd'] == 1:
            crowd_of[s['category_id']] = slot_of[s['id']]
    for p in range(1, P + 1):
        if p_matched[p]:
            continue
        ign = int(conf[0, p])
        if p_cat[p - 1] in crowd_of:
            ign += int(conf[crowd_of[p_cat[p - 1]] + 1, p])
        if not 2 * ign > int(p_area[p]):                  # the integer form of `> 0.5`
            stat[p_cat[p - 1]][1] += 1
    return dict(stat={c: stat[c] for c in categories},
                segments=[(i, c, int(a)) for i, c, a in zip(pid.tolist(), p_cat, p_area[1:].tolist())])


def add_stats(images, categories):
    """PQStat.__iadd__ over the images in order: ((0 + s1) + s2) + ..."""
    total = {c: [0, 0, 0, 0.0] for c in categories}
    for im in images:
        for c in categories:
            for k in range(4):
                total[c][k] += im['stat'][c][k]
    return total


def pq_average(stat, categories, isthing=None):
    """PQStat.pq_average: categories = {id: dict(isthing=0 / 1)}; (dict(pq, sq, rq, n), per class).  n == 0 gives zeros
    (panopticapi divides by n there)."""
    pq = sq = rq = 0.0
    n = 0
    per_class = {}
    for c, info in categories.items():
        if isthing is not None and isthing != (info['isthing'] == 1):
            continue
        tp, fp, fn, iou = stat[c]
        if tp + fp + fn == 0:
            per_class[c] = dict(pq=0.0, sq=0.0, rq=0.0)
            continue
        n += 1
        pq_c = iou / (tp + 0.5 * fp + 0.5 * fn)
        sq_c = iou / tp if tp != 0 else 0
        rq_c = tp / (tp + 0.5 * fp + 0.5 * fn)
        per_class[c] = dict(pq=pq_c, sq=sq_c, rq=rq_c)
        pq += pq_c
        sq += sq_c
        rq += rq_c
    if n == 0:
        return dict(pq=0.0, sq=0.0, rq=0.0, n=0), per_class
    return dict(pq=pq / n, sq=sq / n, rq=rq / n, n=n), per_class


def nine_keys(stat, categories):
    """parse_pq_results: PQ, SQ, RQ, *_th, *_st, each x 100"""
    out = {}
    for suffix, isthing in (('', None), ('_th', True), ('_st', False)):
        r, _ = pq_average(stat, categories, isthing)
        for k in ('pq', 'sq', 'rq'):
            out[k.upper() + suffix] = 100 * r[k]
    return out
