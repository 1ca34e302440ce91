"""
Inputs and expected answers shared by tests/test_rde_cpu.py and tests/test_gpu_rde.py: a transcription of the reference's
ct_utils.get_iou and of its matching rule in Python floats (a second source next to the golden file), the hand-written
structural cases, the threshold pairs and the seeded scenes.
"""

import math

import numpy as np

from megadetector_amd.repeat_detections import BOX_DTYPE


def make_boxes(rows):
    """rows of (x, y, w, h, group, category)"""
    return np.array([tuple(r) for r in rows], dtype=BOX_DTYPE).reshape(-1)


def py_get_iou(bb1, bb2):
    """reference ct_utils.get_iou on [x, y, w, h] boxes, statement for statement"""
    bb1 = [bb1[0], bb1[1], bb1[0] + bb1[2], bb1[1] + bb1[3]]
    bb2 = [bb2[0], bb2[1], bb2[0] + bb2[2], bb2[1] + bb2[3]]
    assert bb1[0] < bb1[2], 'Malformed bounding box (x2 >= x1)'
    assert bb1[1] < bb1[3], 'Malformed bounding box (y2 >= y1)'
    assert bb2[0] < bb2[2], 'Malformed bounding box (x2 >= x1)'
    assert bb2[1] < bb2[3], 'Malformed bounding box (y2 >= y1)'
    x_left = max(bb1[0], bb2[0])
    y_top = max(bb1[1], bb2[1])
    x_right = min(bb1[2], bb2[2])
    y_bottom = min(bb1[3], bb2[3])
    if x_right < x_left or y_bottom < y_top:
        return 0.0
    intersection_area = (x_right - x_left) * (y_bottom - y_top)
    bb1_area = (bb1[2] - bb1[0]) * (bb1[3] - bb1[1])
    bb2_area = (bb2[2] - bb2[0]) * (bb2[3] - bb2[1])
    iou = intersection_area / float(bb1_area + bb2_area - intersection_area)
    assert iou >= 0.0, 'Illegal IOU < 0'
    assert iou <= 1.0, 'Illegal IOU > 1'
    return iou


def py_repeat_detections(boxes, iou_threshold, category_agnostic, occurrence_threshold):
    """the reference's rule (_find_matches_in_directory and the occurrence threshold) on a BOX_DTYPE array, in plain Python:
    (is_candidate, n_instances, pairs) as the C entry points define them"""
    rows = [(float(b['x']), float(b['y']), float(b['w']), float(b['h']), int(b['group']), int(b['category'])) for b in boxes]
    candidates = []                                   # [row, instances]
    for i, b in enumerate(rows):
        found = False
        for cand in candidates:
            c = rows[cand[0]]
            if c[4] != b[4] or (c[5] != b[5] and not category_agnostic):
                continue
            try:
                iou = py_get_iou(b[:4], c[:4])
            except Exception:
                continue
            if iou >= iou_threshold:
                found = True
                cand[1].append(i)
        if not found:
            candidates.append([i, [i]])
    is_candidate = np.zeros(len(rows), np.uint8)
    n_instances = np.zeros(len(rows), np.int32)
    pairs = []
    for row, instances in candidates:
        is_candidate[row] = 1
        n_instances[row] = len(instances)
        if len(instances) >= occurrence_threshold:
            pairs += [(i, row) for i in instances]
    return is_candidate, n_instances, np.array(pairs, np.int64).reshape(-1, 2)


def _chain(n=9):
    # box k matches box k + 1 (IoU 0.818) and not box k + 2 (IoU 0.667)
    return [(0.1 + 0.02 * k, 0.1, 0.2, 0.2, 0, 1) for k in range(n)]


#: name -> (rows, iou threshold, category agnostic, occurrence threshold, is_candidate, n_instances, pairs), written out by hand
STRUCTURAL = {
    # candidates are only ever boxes that matched nothing: 0, 2, 4, 6, 8; box 2k + 1 is an instance of candidate 2k alone
    'drift_chain': (_chain(), 0.8, 0, 2, [1, 0, 1, 0, 1, 0, 1, 0, 1], [2, 0, 2, 0, 2, 0, 2, 0, 1],
                    [(0, 0), (1, 0), (2, 2), (3, 2), (4, 4), (5, 4), (6, 6), (7, 6)]),
    # box 2 lies between candidates 0 and 1 (which do not match each other) and is counted in both
    'two_candidates': ([(0.10, 0.1, 0.2, 0.2, 0, 1), (0.14, 0.1, 0.2, 0.2, 0, 1), (0.12, 0.1, 0.2, 0.2, 0, 1)], 0.8, 0, 2,
                       [1, 1, 0], [2, 2, 0], [(0, 0), (2, 0), (1, 1), (2, 1)]),
    # a candidate and a later box of the same image are two rows like any others
    'same_image': ([(0.3, 0.3, 0.1, 0.1, 0, 1), (0.3, 0.3, 0.1, 0.1, 0, 1)], 0.9, 0, 2, [1, 0], [2, 0], [(0, 0), (1, 0)]),
    # equal boxes in two groups never match
    'two_groups': ([(0.3, 0.3, 0.1, 0.1, 0, 1), (0.3, 0.3, 0.1, 0.1, 1, 1)], 0.9, 0, 1, [1, 1], [1, 1], [(0, 0), (1, 1)]),
    # equal boxes of two categories: apart, and together when the comparison is category agnostic
    'categories': ([(0.3, 0.3, 0.1, 0.1, 0, 1), (0.3, 0.3, 0.1, 0.1, 0, 2)], 0.9, 0, 2, [1, 1], [1, 1], []),
    'categories_agnostic': ([(0.3, 0.3, 0.1, 0.1, 0, 1), (0.3, 0.3, 0.1, 0.1, 0, 2)], 0.9, 1, 2, [1, 0], [2, 0], [(0, 0), (1, 0)]),
    # get_iou raises for w == 0 and w < 0: such a box matches nothing, not even its twin, at any threshold
    'malformed': ([(0.1, 0.1, 0.0, 0.2, 0, 1), (0.1, 0.1, -0.1, 0.2, 0, 1), (0.1, 0.1, 0.0, 0.2, 0, 1), (0.1, 0.1, 0.2, 0.2, 0, 1),
                   (0.1, 0.1, -0.1, 0.2, 0, 1)], 0.0, 0, 2, [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], []),
    'empty': ([], 0.9, 0, 1, [], [], []),
    'one': ([(0.3, 0.3, 0.1, 0.1, 0, 1)], 0.9, 0, 1, [1], [1], [(0, 0)]),
    # three instances: suspicious at a threshold of exactly 3, not at 4
    'threshold_at_count': ([(0.3, 0.3, 0.1, 0.1, 0, 1)] * 3, 0.9, 0, 3, [1, 0, 0], [3, 0, 0], [(0, 0), (1, 0), (2, 0)]),
    'threshold_above_count': ([(0.3, 0.3, 0.1, 0.1, 0, 1)] * 3, 0.9, 0, 4, [1, 0, 0], [3, 0, 0], []),
}


def structural(name):
    rows, thr, agnostic, occ, is_cand, n_inst, pairs = STRUCTURAL[name]
    return (make_boxes(rows), thr, agnostic, occ, np.array(is_cand, np.uint8), np.array(n_inst, np.int32),
            np.array(pairs, np.int64).reshape(-1, 2))


def threshold_pairs(n=200, seed=5):
    """n pairs of overlapping boxes in full double precision with their IoU as py_get_iou computes it: with the threshold set
    to exactly that IoU the second box matches the first, with the next double above it it does not.  A contracted
    multiply-add, a reciprocal or a rewritten comparison moves the last bit of some of them."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x, y, w, h = rng.uniform(0.05, 0.5, 4)
        dx, dy = rng.uniform(-0.3, 0.3, 2) * (w, h)
        sw, sh = rng.uniform(0.7, 1.3, 2)
        a = (float(x), float(y), float(w), float(h))
        b = (float(x + dx), float(y + dy), float(w * sw), float(h * sh))
        iou = py_get_iou(b, a)
        if 0.05 < iou < 1.0:
            out.append((make_boxes([a + (0, 1), b + (0, 1)]), iou))
    return out


def seeded_scene(n_groups, per_group, seed, decimals=None):
    """Groups of boxes from drifting clusters: a cluster's box moves on a little with every appearance, so that chains (a box
    that matches the box before it and not the cluster's candidate) and boxes between two candidates occur; categories 1 .. 3,
    a few malformed boxes."""
    rng = np.random.default_rng(seed)
    rows = []
    for g in range(n_groups):
        n = per_group + int(rng.integers(0, 37))
        clusters = [[rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.6), rng.uniform(0.1, 0.3), rng.uniform(0.1, 0.3),
                     int(rng.integers(1, 4)), rng.uniform(0.0005, 0.004)] for _ in range(12)]
        for i in range(n):
            u = rng.random()
            if u < 0.85:
                c = clusters[int(rng.integers(0, len(clusters)))]
                c[0] += c[5] * rng.uniform(0.0, 2.0)
                if c[0] > 0.65:
                    c[0] = 0.05
                row = (c[0] + rng.normal(0, 0.002), c[1] + rng.normal(0, 0.002), c[2], c[3], g, c[4] if rng.random() < 0.9 else 1)
            elif u < 0.98:
                w, h = rng.uniform(0.03, 0.5, 2)
                row = (rng.uniform(0, 1 - w), rng.uniform(0, 1 - h), w, h, g, int(rng.integers(1, 4)))
            else:
                row = (0.4, 0.4, -0.1 if rng.random() < 0.5 else 0.0, 0.2, g, 1)
            if decimals is not None:
                row = tuple(round(float(v), decimals) for v in row[:4]) + row[4:]
            rows.append(row)
    return make_boxes(rows)


def has_multi_match(pairs):
    """a box that is an instance of two candidates"""
    return len(pairs) > 0 and np.unique(pairs[:, 0], return_counts=True)[1].max() > 1


def has_chain(boxes, is_candidate, iou_threshold):
    """a candidate that matches an earlier box of its group which is no candidate (so that box matched something else): the
    drift-chain situation, where comparing against every earlier box instead of every earlier candidate goes wrong"""
    cand = np.flatnonzero(is_candidate)
    for c in cand.tolist():
        b = boxes[c]
        lo = c - 1
        while lo >= 0 and boxes[lo]['group'] == b['group']:
            if not is_candidate[lo] and boxes[lo]['category'] == b['category']:
                try:
                    if py_get_iou([b['x'], b['y'], b['w'], b['h']], [boxes[lo]['x'], boxes[lo]['y'], boxes[lo]['w'], boxes[lo]['h']]) >= iou_threshold:
                        return True
                except Exception:
                    pass
            lo -= 1
            if c - lo > 400:
                break
    return False


def next_up(x):
    return math.nextafter(x, 2.0)
