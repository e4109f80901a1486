"""TEST ORACLE: sliced inference on large scenes, restated loop by loop on numpy / plain Python.

What the reference's large-image path computes (demo/large_image_demo.py, mmdet/utils/large_image.py) goes through two
libraries that are not installed here; their semantics are restated from their documented behaviour:
  sahi.slicing.get_slice_bboxes (auto_slice_resolution=False)   -> slice_bboxes
  sahi.slicing.shift_bboxes / shift_masks                       -> shift_bboxes / shift_masks
  pycocotools.mask.encode (maskApi.c rleEncode)                 -> rle_counts
and the run-domain form of shift_masks + rleEncode that `rsp_rle_shift` implements -> rle_shift_counts (the definition
of the kernel's header comment, one pixel-stream segment at a time; used where a dense scene canvas would not fit).
Nothing here imports the package under test."""
import numpy as np


def slice_bboxes(height, width, slice_height, slice_width, overlap_height_ratio, overlap_width_ratio):
    out = []
    y_max = y_min = 0
    y_overlap = int(overlap_height_ratio * slice_height)
    x_overlap = int(overlap_width_ratio * slice_width)
    while y_max < height:
        x_min = x_max = 0
        y_max = y_min + slice_height
        while x_max < width:
            x_max = x_min + slice_width
            if y_max > height or x_max > width:
                xmax = min(width, x_max)
                ymax = min(height, y_max)
                xmin = max(0, xmax - slice_width)
                ymin = max(0, ymax - slice_height)
                out.append([xmin, ymin, xmax, ymax])
            else:
                out.append([x_min, y_min, x_max, y_max])
            x_min = x_max - x_overlap
        y_min = y_max - y_overlap
    return out


def shift_bboxes(bboxes, offset):
    """fp32 boxes [n, 4] + (ox, oy, ox, oy)"""
    b = np.asarray(bboxes, np.float32).reshape(-1, 4)
    return b + np.asarray([offset[0], offset[1], offset[0], offset[1]], np.float32)


def shift_masks(masks, offset, full_shape):
    """masks [n, h, w] -> [n, H, W]: every tile mask placed at [oy:oy + h, ox:ox + w] of a zero canvas"""
    masks = np.asarray(masks).astype(bool)
    n, h, w = masks.shape
    H, W = full_shape
    ox, oy = offset
    out = np.zeros((n, H, W), bool)
    out[:, oy:oy + h, ox:ox + w] = masks
    return out


def rle_counts(mask):
    """maskApi.c rleEncode on one [H, W] mask: run lengths of the column-major stream, the first run counts zeros"""
    flat = np.asarray(mask).astype(np.uint8).T.reshape(-1)           # column-major stream
    cnts, p, c = [], 0, 0
    for v in flat.tolist():
        if v != p:
            cnts.append(c)
            c = 0
            p = v
        c += 1
    cnts.append(c)
    return cnts


def rle_counts_np(mask):
    """rle_counts without the per-pixel loop (for scene-sized masks): run boundaries from the stream's value changes.  The
    CPU tier checks it against rle_counts."""
    flat = np.asarray(mask).astype(np.uint8).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.size]])
    cnts = np.diff(edges).tolist()
    if flat.size and flat[0]:
        cnts.insert(0, 0)
    return cnts


def _append_run(runs, value, length):
    """runs: list of [value, length]; adjacent runs of one value merge, zero-length insertions insert nothing"""
    if length == 0:
        return
    if runs and runs[-1][0] == value:
        runs[-1][1] += length
    else:
        runs.append([value, length])


def rle_shift_counts(counts, h, w, offset, full_shape):
    """run counts of an [h, w] mask -> run counts of the mask placed at (ox, oy) in (H, W), in the run domain: ox*H + oy
    zeros; the tile's stream with H - h zeros inserted after every tile column (H - h - oy after the last); then
    (W - ox - w) * H zeros."""
    H, W = full_shape
    ox, oy = offset
    runs = []
    _append_run(runs, 0, ox * H + oy)
    col_left = h                                                      # pixels left in the current tile column
    col = 0
    for i, c in enumerate(counts):
        v = i & 1
        while c > 0:
            take = min(c, col_left)
            _append_run(runs, v, take)
            c -= take
            col_left -= take
            if col_left == 0:
                col += 1
                _append_run(runs, 0, (H - h) if col < w else (H - h - oy))
                col_left = h
    assert col == w and col_left == h, 'the counts do not describe an [h, w] mask'
    _append_run(runs, 0, (W - ox - w) * H)
    if not runs or runs[0][0] == 1:
        runs.insert(0, [0, 0])                                        # the first count is a count of zeros
    return [r[1] for r in runs]


def counts_to_mask(counts, h, w):
    flat = np.zeros(h * w, np.uint8)
    p = 0
    for i, c in enumerate(counts):
        if i & 1:
            flat[p:p + c] = 1
        p += c
    return flat.reshape(w, h).T.astype(bool)


def merge(tile_results, offsets, full_shape, batched_nms, iou_thr):
    """mmdet/utils/large_image.py:27-104 on numpy/torch data.  tile_results: list of dict(bboxes [n, 4] fp32, scores [n],
    labels [n]) per tile; batched_nms(boxes, scores, labels, thr) -> (dets, keep) is handed in (oracle.glue.batched_nms).
    Returns (keep indices into the tile-ordered concatenation, shifted boxes, scores, labels, tile index)."""
    import torch
    boxes = np.concatenate([shift_bboxes(r['bboxes'], o) for r, o in zip(tile_results, offsets)], 0)
    scores = np.concatenate([np.asarray(r['scores'], np.float32) for r in tile_results], 0)
    labels = np.concatenate([np.asarray(r['labels'], np.int64) for r in tile_results], 0)
    tile = np.concatenate([np.full(len(r['scores']), i, np.int64) for i, r in enumerate(tile_results)], 0)
    _, keep = batched_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(labels), iou_thr)
    return keep.numpy(), boxes, scores, labels, tile
