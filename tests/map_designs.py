"""Designed inputs for the detection metric (csrc/vtd_metrics.hip: map_update_kernel with
image_record, map_result_kernel, iou_kernel): cases that reach every branch by construction, a
branch walker that names what each case reaches, and wrong restatements (mutants) that the cases
must tell apart from the right one.  Pure numpy, importable without a GPU;
tests/test_map_designs_host.py checks this module on the CPU, tests/test_gpu_metrics.py runs the
same cases on the device.

Why: the seeded fuzz of tests/map_cases.random_batch never has 14 positive predictions of one
class in one image (most: 9) nor more than 7 hits, so it runs neither scenario c's sort and cut,
nor the 14-hit exit, nor the sort and cut of the left-overs, nor two labels of equal area
(`fuzz_replay` below counts it; the host test asserts it).

The walker.  `walk(label, pred, category)` restates one image x one category of update_state
(vision_transformer_detector.py:1480-1852) on its own, in float32 scalars, and returns
(related, label count, 14 (confidence, IoU) entries, tags).  `Walked` is the whole metric on top
of it, written the way the kernel works (per class: the latest three related images of a batch,
one shift by their number) and tags what the state update and result() did.  The host test holds
both to oracle/vtd_map.py on every designed case and on the fuzz, so they cannot drift.

Tags (TAGS): what image_record did
  b                  labels, no positive prediction: 14 zero entries
  c_under/_exact/_over  positive predictions, no label: n < 14 order kept and zeros at the end;
                     n == 14 sorted descending; n > 14 sorted and cut to 14
  d_hit / d_miss     greedy matching: a label's best IoU is > 0.5 / is not
  d_tie_hit          several predictions are isclose to the best IoU and are all masked
  d_area_order       the ascending-area order of the labels differs from their row order
  d_area_tie         two labels of bit-equal area (the stable order decides who matches first)
  d_full             14 hits: break, left-over predictions dropped
  d_left_fit         hits + left-overs <= 14: appended in row order, no sort
  d_left_cut         hits + left-overs > 14: left-overs sorted descending, cut to 14 - hits
  d_fifo_front_zero  fewer than 14 entries appended: zeros stay in front
what the state update did (per class and update_state call)
  s_shift1/2/3       1, 2, 3 related images pushed onto a non-empty state of the class
  s_over3            more than 3 related images in one batch: only the latest 3 are kept
  s_beyond_256       a kept image has an index >= 256 (past one stride of the 256 threads)
what result() did (per class)
  r_full             all 42 entries have confidence > 0
  r_conf_tie         equal confidences in different slots with different IoUs
  r_iou_eq_thr       an IoU bit-equal to a threshold: a true positive below it, not at it
  r_pred_only        no label in the state but predictions: AP 0, counted in the mean
  r_label_only       labels and no prediction: AP 0

Values.  Everything is built from the reference's standard object (tests/map_cases.BOX:
objectness 1, class 79, a 10 x 10 box at 10.2).  A class is k + j / 256 with 0 <= j < 64, whose
float32 class confidence (0.5 - j / 256) / 0.5 = 1 - j / 128 is exact, finite and > 0.5
(`confidence`, asserted).  The matching cases put the object on a dyadic grid (`cell`): labels 32
high, a prediction with the label's centre and width and height hp, so that every edge, area and
product is an integer and IoU = hp / 32 is exact; tests/test_map_kat.py derives four of them by
hand from the reference's text.  The threshold case keeps the object at 10.2.

Out of scope: non-finite predictions and label classes that are not integers.
"""
from collections import Counter

import numpy as np

from tests.map_cases import BOX, random_batch

F = np.float32
CLASSES, LATEST, P = 80, 3, 14
K = int(BOX[1])                                  # the standard object's class, 79

WALK_TAGS = ("b", "c_under", "c_exact", "c_over", "d_hit", "d_miss", "d_tie_hit", "d_area_order",
             "d_area_tie", "d_full", "d_left_fit", "d_left_cut", "d_fifo_front_zero")
STATE_TAGS = ("s_shift1", "s_shift2", "s_shift3", "s_over3", "s_beyond_256")
RESULT_TAGS = ("r_full", "r_conf_tie", "r_iou_eq_thr", "r_pred_only", "r_label_only")
TAGS = WALK_TAGS + STATE_TAGS + RESULT_TAGS

MUTANTS = {
    "c_never_sorts": "scenario c keeps the row order for n >= 14 too",
    "c_first_14": "scenario c keeps the first 14 (then sorts them) instead of the top 14",
    "no_break": "no break at 14 hits: later hits push the first ones out",
    "left_unsorted": "left-overs are cut to 14 - hits without the sort",
    "left_cut_14": "left-overs are cut to 14 instead of 14 - hits",
    "label_index_order": "labels are matched in row order instead of ascending area",
    "area_unstable": "the area sort reverses ties",
    "result_unstable": "result()'s confidence sort reverses ties",
    "iou_ge_thr": "result() counts iou >= thr as a true positive",
    "first_256": "the latest-three search sees only the first 256 images of a batch",
}


# ------------------------------------------------------------------ float32 scalar pieces
def confidence(cls):
    """(0.5 - |c - round(c)|) / 0.5, round half to even (vtd.py:1367-1376)."""
    c = F(cls)
    return F((F(0.5) - abs(c - F(np.rint(c)))) / F(0.5))


def isclose(a, b):
    """tf.experimental.numpy.isclose: |a - b| <= 1e-8 + 1e-5 |b|."""
    return bool(abs(F(a) - F(b)) <= F(1e-8) + F(1e-5) * abs(F(b)))


def positive(row):
    """vtd.py:1458-1463."""
    return bool(F(row[0]) > F(0.5) and confidence(row[1]) > F(0.5))


def iou(l, p):
    """iou_calculator (vtd.py:761-875) for one pair of (x, y, height, width) boxes."""
    lx, ly, lh, lw = (F(v) for v in l)
    px, py, ph, pw = (F(v) for v in p)
    two = F(2)
    ll, lr, pl, pr = lx - lw / two, lx + lw / two, px - pw / two, px + pw / two
    lt, lb, pt, pb = ly - lh / two, ly + lh / two, py - ph / two, py + ph / two
    ih = iw = F(0)
    if ll < pr and lr > pl and lt < pb and lb > pt:
        ih, iw = min(lb, pb) - max(lt, pt), min(lr, pr) - max(ll, pl)
    inter = F(ih * iw)
    union = F(F(F(pw * ph) + F(lw * lh)) - inter)
    return F(inter / F(union + F(1e-8)))


def thresholds():
    """tf.linspace(0.5, 0.95, 10) in float32: start + i * step, the last element is stop."""
    step = F((F(0.95) - F(0.5)) / F(9))
    return [F(F(0.5) + step * F(i)) for i in range(9)] + [F(0.95)]


def _desc(values, reverse_ties=False):
    """Indices by descending value; ties keep the lower index first (tf.sort / tf.argsort are
    top_k based), or the higher one for the unstable mutants."""
    return sorted(range(len(values)),
                  key=lambda i: (-float(values[i]), -i if reverse_ties else i))


# ------------------------------------------------------------------ the walker
def walk(label, pred, category, mutant=None):
    """One image x one category (vtd.py:1480-1852): (related, count, entries, tags)."""
    label, pred = np.asarray(label, F), np.asarray(pred, F)
    fc = F(category)
    lmask = [isclose(r[1], fc) for r in label]
    pmask = [positive(r) and isclose(F(np.rint(r[1])), fc) for r in pred]
    count, tags = sum(lmask), set()
    zero = (F(0), F(0))
    if not (any(lmask) or any(pmask)):                   # scenario a
        return False, 0, None, tags
    if not any(pmask):                                   # scenario b, vtd.py:1552-1556
        return True, count, [zero] * P, {"b"}
    if not any(lmask):                                   # scenario c, vtd.py:1560-1621
        confs = [confidence(r[1]) for r, m in zip(pred, pmask) if m]
        n = len(confs)
        tags.add("c_under" if n < P else "c_exact" if n == P else "c_over")
        if n < P:
            confs = confs + [F(0)] * (P - n)
        elif mutant == "c_never_sorts":
            confs = confs[:P]
        elif mutant == "c_first_14":
            confs = [confs[i] for i in _desc(confs[:P])]
        else:
            confs = [confs[i] for i in _desc(confs)][:P]
        return True, count, [(c, F(0)) for c in confs], tags
    # scenario d, vtd.py:1625-1852
    gone = (F(-8),) * 4
    boxes = [tuple(r[2:]) if m else gone for r, m in zip(pred, pmask)]
    labs = [r[2:] for r, m in zip(label, lmask) if m]
    areas = [F(b[3] * b[2]) for b in labs]
    rows = list(range(len(labs)))
    if mutant == "label_index_order":
        order = rows
    else:                                                # tf.argsort ASCENDING, lower row first
        order = sorted(rows, key=lambda i: (float(areas[i]),
                                            -i if mutant == "area_unstable" else i))
    if order != rows:
        tags.add("d_area_order")
    if len(set(float(a) for a in areas)) < len(areas):
        tags.add("d_area_tie")
    appended, hits = [], 0
    for li in order:
        ious = [iou(labs[li], b) for b in boxes]
        best = max(ious)
        if best > F(0.5):                                # vtd.py:1689
            hits += 1
            tied = [j for j, v in enumerate(ious) if isclose(v, best)]
            tags.add("d_hit")
            if len(tied) > 1:
                tags.add("d_tie_hit")
            appended.append((confidence(pred[tied[0]][1]), best))
            for j in tied:
                boxes[j] = gone
        else:
            tags.add("d_miss")
        if hits == P and mutant != "no_break":           # vtd.py:1756-1758
            tags.add("d_full")
            break
    left = [confidence(pred[i][1]) for i, b in enumerate(boxes) if all(v >= 0 for v in b)]
    if left and hits < P:                                # vtd.py:1785-1788
        if hits + len(left) > P:                         # vtd.py:1809-1827
            tags.add("d_left_cut")
            keep = P if mutant == "left_cut_14" else P - hits
            if mutant != "left_unsorted":
                left = [left[i] for i in _desc(left)]
            left = left[:keep]
        else:
            tags.add("d_left_fit")
        appended += [(c, F(0)) for c in left]
    if len(appended) < P:
        tags.add("d_fifo_front_zero")
    return True, count, ([zero] * P + appended)[-P:], tags


class Walked:
    """The whole metric on top of `walk`, organised like the kernels: per class, the latest
    three related images of a batch and one shift by their number; result() per threshold and
    class.  `counts` has how many (image, class) records or classes reached each tag."""

    def __init__(self, mutant=None):
        self.mutant = mutant
        self.counts = Counter()
        self.records = 0
        self.reset_state()

    def reset_state(self):
        self.latest_positive_bboxes = np.zeros((CLASSES, LATEST, P, 2), F)
        self.labels_quantity_per_image = np.zeros((CLASSES, LATEST), F)
        self.showed_up_classes = np.zeros(CLASSES, bool)
        self._pushed = np.zeros(CLASSES, int)

    @property
    def tags(self):
        return set(self.counts)

    def update_state(self, y_true, y_pred):
        y_true, y_pred = np.asarray(y_true, F), np.asarray(y_pred, F)
        related = {}
        for b in range(y_true.shape[0]):
            cand = set()
            for r in y_true[b]:
                if r[1] >= 0:
                    cand.add(int(np.rint(r[1])))
            for r in y_pred[b]:
                if positive(r):
                    cand.add(int(np.rint(r[1])))
            for c in sorted(cand):
                if not 0 <= c < CLASSES:
                    continue
                rel, count, entries, tags = walk(y_true[b], y_pred[b], c, self.mutant)
                if rel:
                    self.records += 1
                    self.counts.update(tags)
                    related.setdefault(c, []).append((b, count, entries))
        for c, recs in related.items():
            self.showed_up_classes[c] = True             # vtd.py:1343-1411
            if self.mutant == "first_256":
                recs = [r for r in recs if r[0] < 256]
            if len(recs) > LATEST:
                self.counts["s_over3"] += 1
            recs = recs[-LATEST:]
            k = len(recs)
            if k == 0:
                continue
            if self._pushed[c]:
                self.counts["s_shift%d" % k] += 1
            if any(r[0] >= 256 for r in recs):
                self.counts["s_beyond_256"] += 1
            self._pushed[c] += k
            lq, bb = self.labels_quantity_per_image[c], self.latest_positive_bboxes[c]
            lq[k:], bb[k:] = lq[:LATEST - k].copy(), bb[:LATEST - k].copy()
            for slot, (_, count, entries) in enumerate(reversed(recs)):   # newest in slot 0
                lq[slot], bb[slot] = count, np.array(entries, F)

    def category_ap(self, c, thr, tag=False):
        """vtd.py:1886-2007 for one class and one IoU threshold."""
        ent = self.latest_positive_bboxes[c].reshape(-1, 2)
        lq = F(0)
        for v in self.labels_quantity_per_image[c]:
            lq = F(lq + v)
        rp, tp, fp = [F(1)], F(0), F(0)
        for i in _desc(ent[:, 0], self.mutant == "result_unstable"):
            conf, v = ent[i]
            if not conf > 0:
                continue
            if v > thr or (self.mutant == "iou_ge_thr" and v == thr):
                tp = F(tp + F(1))
                rp.append(F(tp / F(tp + fp)))
            else:
                fp = F(fp + F(1))
                rp[-1] = F(tp / F(tp + fp))
        if tag:
            live = [(i // P, float(e[0]), float(e[1])) for i, e in enumerate(ent) if e[0] > 0]
            if len(live) == LATEST * P:
                self.counts["r_full"] += 1
            if any(a[1] == b[1] and a[0] != b[0] and a[2] != b[2] for a in live for b in live):
                self.counts["r_conf_tie"] += 1
            if any(e[2] == float(t) for e in live for t in thresholds()):
                self.counts["r_iou_eq_thr"] += 1
            if live and not lq > 0:
                self.counts["r_pred_only"] += 1
            if lq > 0 and not live:
                self.counts["r_label_only"] += 1
        if not lq > 0 or len(rp) == 1:
            return F(0)
        acc = F(0)
        for a, b in zip(rp, rp[1:]):
            acc = F(acc + F(a + b))
        return F(F(acc * F(F(1) / lq)) / F(2))

    def per_iou(self, tag=True):
        out = []
        for t, thr in enumerate(thresholds()):
            aps = [self.category_ap(c, thr, tag and t == 0)
                   for c in range(CLASSES) if self.showed_up_classes[c]]
            s = F(0)
            for a in aps:
                s = F(s + a)
            out.append(F(s / F(len(aps))) if aps else F(0))
        return out

    def result(self):
        s = F(0)
        for a in self.per_iou(tag=False):
            s = F(s + a)
        return F(s / F(10))


def fuzz_batches():
    """The exact inputs of test_map_random_batches_match_oracle and
    test_map_batch_larger_than_block in tests/test_gpu_metrics.py: one list of batches per
    metric object."""
    runs = []
    for seed, classes in ((0, (0, 80)), (1, (0, 3)), (2, (77, 80)), (3, (0, 1))):
        rng = np.random.default_rng(seed)
        runs.append([random_batch(rng, batch, boxes=17, classes=classes) for batch in (5, 1, 9)])
    runs.append([random_batch(np.random.default_rng(7), 600, boxes=8, classes=(0, 4))])
    return runs


def fuzz_replay():
    """(records, Counter of tags) over `fuzz_batches`."""
    counts, records = Counter(), 0
    for run in fuzz_batches():
        m = Walked()
        for y, p in run:
            m.update_state(y, p)
        m.per_iou()
        counts.update(m.counts)
        records += m.records
    return records, counts


# ------------------------------------------------------------------ building blocks
def cls(k, j):
    """Class k + j / 256: confidence exactly 1 - j / 128."""
    assert 0 <= j < 64
    c = F(F(k) + F(j) / F(256))
    assert np.isfinite(c) and confidence(c) == F(1 - j / 128) > F(0.5) and np.rint(c) == k
    return c


def cell(i):
    """Centre of grid cell i < 64: 64 apart, so boxes up to 48 wide and high never touch."""
    assert 0 <= i < 64
    return 32.0 + 64.0 * (i % 8), 32.0 + 64.0 * (i // 8)


def std(i):
    """The standard object's box moved to cell i: (x, y, height, width)."""
    return BOX[2] + 64.0 * (i % 8), BOX[3] + 64.0 * (i // 8), BOX[4], BOX[5]


def row(c, x, y, h, w, obj=BOX[0]):
    return obj, c, x, y, h, w


def blank(batch, nb):
    """Empty labels (class and box -8, as the reference marks them) and predictions of
    objectness 0, which are never positive."""
    y = np.full((batch, nb, 6), -8.0, F)
    y[..., 0] = 0.0
    return y, np.zeros((batch, nb, 6), F)


def clutter(p, b, first, k=K - 1):
    """Fills the prediction rows from `first` on with positive predictions of another class
    on the far cells: rows that image_record must turn into -8 boxes for class K."""
    for n, i in enumerate(range(first, p.shape[1])):
        p[b, i] = row(cls(k, n % 64), *std(63 - n % 40))


H = 32.0                                             # designed labels' height


def matched(y, p, b, lrow, prow, i_cell, w, hp, j, k=K):
    """Label (32 high, w wide) in cell i_cell and a prediction with its centre and width, hp
    high: the prediction lies inside the label, IoU = hp w / (32 w) = hp / 32 exactly."""
    x, yy = cell(i_cell)
    y[b, lrow] = row(float(k), x, yy, H, w)
    p[b, prow] = row(cls(k, j), x, yy, hp, w)
    assert iou(y[b, lrow, 2:], p[b, prow, 2:]) == F(hp / 32)


# ------------------------------------------------------------------ the designed cases
def image_c(p, b, n, tie_at_cut=False):
    """n positive predictions of class K, no label.  Confidence index j of row i is
    (11 i + 3) mod n: distinct and out of order; with `tie_at_cut` the 14th and 15th largest
    confidences are equal (j = 13 twice)."""
    for i in range(n):
        j = (11 * i + 3) % n
        if tie_at_cut and j >= 14:
            j -= 1
        p[b, i] = row(cls(K, j), *std(i))


def case_scenario_c(nb):
    """13, 14 and nb positive predictions in three images, then one with a tie at the cut."""
    y, p = blank(3, nb)
    for b, n in enumerate((13, 14, nb)):
        image_c(p, b, n)
    y2, p2 = blank(1, nb)
    image_c(p2, 0, nb, tie_at_cut=True)
    return [(y, p), (y2, p2)], {"c_under", "c_exact", "c_over"}


def image_d_full(y, p, b, extras):
    """min(16, rows) labels of class K.  Label i is 8 + rank(i) wide with rank(i) =
    (m i + 3) mod n (m = 5 for 16 labels): distinct areas, not in row order.  Its prediction
    (row i) is 17 + i high, IoU (17 + i) / 32 > 0.5, confidence 1 - i / 128.  `extras` more
    positive predictions of the class on cells of their own match nothing."""
    nb = y.shape[1]
    n = min(16, nb)
    m = {16: 5, 15: 4}[n]
    for i in range(n):
        matched(y, p, b, i, i, i, 8.0 + (m * i + 3) % n, 17.0 + i, i)
    for e in range(min(extras, nb - n)):
        p[b, n + e] = row(cls(K, 40 + e % 20), *cell(n + e), H, 16.0)


def case_d_full(nb):
    """16 labels (15 where there are only 15 rows), every one with a prediction above 0.5:
    the 14 smallest take the entries, the count is 16, the other predictions are dropped."""
    y, p = blank(1, nb)
    image_d_full(y, p, 0, extras=20)
    return [(y, p)], {"d_full", "d_hit", "d_area_order"}


HP_CUT = (32.0, 31.0, 24.0, 20.0, 17.0)              # IoU 1, 31/32, 3/4, 5/8, 17/32


def image_d_cut(y, p, b, hits, left):
    """`hits` labels of class K in rows 0.., label j 12 - j wide (area order is the reverse
    of the row order), its prediction HP_CUT[j] high with confidence 1 - (20 + j) / 128, in
    row left + j.  Rows 0..left-1 hold predictions that match nothing; row i has the
    (7 i + 3) mod left -th largest confidence: 1 - m / 128, or 1 - (m + 5) / 128 from m = 20."""
    for j in range(hits):
        matched(y, p, b, j, left + j, j, 12.0 - j, HP_CUT[j], 20 + j)
    for i in range(left):
        m = (7 * i + 3) % left
        p[b, i] = row(cls(K, m if m < 20 else m + 5), *cell(hits + i), H, 16.0)


def case_d_cut(nb):
    """hits + left-overs == 14 (kept in order), == 15 and well above (sorted, cut to
    14 - hits).  5 hits; 3 where 5 + 12 rows do not fit.  At 64 rows the last image fills
    every row."""
    hits = 5 if nb >= 17 else 3
    y, p = blank(3, nb)
    for b, left in enumerate((P - hits, P + 1 - hits, 12 if nb < 64 else nb - hits)):
        image_d_cut(y, p, b, hits, left)
    return [(y, p)], {"d_left_fit", "d_left_cut", "d_hit", "d_area_order"}


def image_equal_areas(y, p, b):
    """Labels A (row 0, y in [64, 96]) and B (row 1, y in [68, 100]), both 32 x 32 at x = 80:
    bit-equal areas.  Predictions P2 (row 0, y in [72, 104]) and P1 (row 1, y in [65, 97]), same
    x and width.  Both labels like P1 best (A 31/33, B 29/35; P2: A 24/40, B 28/36).  The
    stable order lets A take P1 and leaves P2 to B; reversed, B takes P1 and A gets P2 at
    24/40.  Label C (row 2, 16 x 16, its own cell) is smaller and is matched first."""
    y[b, 0] = row(float(K), 80.0, 80.0, H, 32.0)
    y[b, 1] = row(float(K), 80.0, 84.0, H, 32.0)
    p[b, 0] = row(cls(K, 0), 80.0, 88.0, H, 32.0)
    p[b, 1] = row(cls(K, 1), 80.0, 81.0, H, 32.0)
    x, yy = cell(5)
    y[b, 2] = row(float(K), x, yy, 16.0, 16.0)
    p[b, 2] = row(cls(K, 2), x, yy, 16.0, 16.0)
    a, bb, p2, p1 = y[b, 0, 2:], y[b, 1, 2:], p[b, 0, 2:], p[b, 1, 2:]
    assert F(a[2] * a[3]) == F(bb[2] * bb[3])
    assert iou(a, p1) > iou(a, p2) > F(0.5) and iou(bb, p1) > iou(bb, p2) > F(0.5)
    assert iou(a, p2) != iou(bb, p2)


def case_equal_areas(nb):
    y, p = blank(1, nb)
    image_equal_areas(y, p, 0)
    clutter(p, 0, 3)
    return [(y, p)], {"d_area_tie", "d_area_order", "d_hit", "d_fifo_front_zero"}


def case_tie_at_max(nb):
    """Label L (32 x 32) and two identical predictions of it (rows 2 and nb - 1) plus one wider by
    2^-15 (row 5; IoU 1 - 2^-20, not equal and still isclose): all three are masked, the
    first one's confidence is recorded.  Label M (40 high, same centre) would match any of them
    at 0.8 and finds none."""
    y, p = blank(1, nb)
    y[0, 0] = row(float(K), 80.0, 80.0, H, 32.0)
    y[0, 1] = row(float(K), 80.0, 80.0, 40.0, 32.0)
    p[0, 2] = row(cls(K, 3), 80.0, 80.0, H, 32.0)
    p[0, nb - 1] = row(cls(K, 7), 80.0, 80.0, H, 32.0)
    p[0, 5] = row(cls(K, 9), 80.0, 80.0, H, 32.0 + 2.0 ** -15)
    near = iou(y[0, 0, 2:], p[0, 5, 2:])
    assert near < F(1) and isclose(near, F(1)) and iou(y[0, 1, 2:], p[0, 2, 2:]) == F(0.8)
    clutter(p, 0, 6)
    p[0, nb - 1] = row(cls(K, 7), 80.0, 80.0, H, 32.0)
    return [(y, p)], {"d_tie_hit", "d_hit", "d_miss", "d_fifo_front_zero"}


def case_thresholds():
    """Either side of every comparison that makes a prediction positive or a match a hit."""
    y, p = blank(2, 10)
    y[0, 0] = row(5.0, *std(0))
    p[0, 0] = row(5.0, *std(0), obj=0.5)                 # objectness not > 0.5
    p[0, 1] = row(5.25, *std(0))                         # confidence exactly 0.5
    p[0, 2] = row(4.5, *std(0))                          # rounds to 4 (half to even), confidence 0
    p[0, 3] = row(5.5, *std(0))                          # rounds to 6, confidence 0
    assert confidence(5.25) == F(0.5) and confidence(4.5) == 0 and confidence(5.5) == 0
    assert np.rint(F(4.5)) == 4 and np.rint(F(5.5)) == 6
    y[0, 1] = row(0.0, *std(1))
    p[0, 4] = row(-0.2, *std(1))                         # rounds to -0: category 0, positive
    assert np.rint(F(-0.2)) == 0 and np.signbit(np.rint(F(-0.2))) and positive(p[0, 4])
    y[0, 3] = row(float(K), *std(3))
    p[0, 5] = row(79.6, *std(3))                         # rounds to 80, confidence 0.2
    p[0, 6] = row(79.8, *std(3))                         # positive, category 80: no class has it
    assert not positive(p[0, 5]) and positive(p[0, 6]) and np.rint(F(79.8)) == CLASSES
    x, yy = cell(2)
    y[0, 2] = row(7.0, x, yy, H, 32.0)
    p[0, 7] = row(cls(7, 1), x, yy, 16.0, 32.0)          # IoU exactly 0.5: not a hit
    assert iou(y[0, 2, 2:], p[0, 7, 2:]) == F(0.5)
    y[1, 0] = row(5.0, *std(0))                          # one float32 step past both thresholds
    p[1, 0] = row(np.nextafter(F(5.25), F(5)), *std(0), obj=np.nextafter(F(0.5), F(1)))
    assert positive(p[1, 0])
    return [(y, p)], {"b", "d_hit", "d_miss", "d_left_fit", "d_fifo_front_zero"}


def _seen(y, p, b, t, k=K):
    """Image b relates to class k: a standard object and its prediction of confidence
    1 - t / 128 in row 0."""
    y[b, 0] = row(float(k), *std(0))
    p[b, 0] = row(cls(k, t % 64), *std(0))


def case_state_calls():
    """Class K sees 1, 2, 3, 5, 1 and 2 related images in six update_state calls, every one
    with a confidence of its own: shifts by 1, 2 and 3 onto a non-empty state, and 5 in one
    batch of which the first two are lost.  The other images relate to class 3 or to none."""
    batches, t = [], 0
    for size, where in ((3, (1,)), (4, (0, 3)), (5, (0, 2, 4)), (7, (0, 1, 3, 5, 6)), (2, (0,)),
                        (4, (1, 2))):
        y, p = blank(size, 3)
        for b in range(size):
            if b in where:
                _seen(y, p, b, t)
                t += 1
            elif b % 2:
                y[b, 1] = row(3.0, *std(1))
        batches.append((y, p))
    return batches, {"s_shift1", "s_shift2", "s_shift3", "s_over3", "d_hit", "b"}


def case_state_600():
    """A small batch, then 600 images of 2 boxes.  Only images 0, 255, 256 and 599 relate to
    class K: the latest three are 599, 256, 255, on both sides of the 256-thread stride.  Class
    5 is in 255 and 256 only, class 6 in 0, class 7 in 599; all others relate to class 3."""
    y0, p0 = blank(2, 2)
    _seen(y0, p0, 0, 40)
    _seen(y0, p0, 1, 41)
    y, p = blank(600, 2)
    for t, b in enumerate((0, 255, 256, 599)):
        _seen(y, p, b, t)
    for b in range(600):
        if y[b, 0, 1] < 0:
            _seen(y, p, b, b, k=3)
    for b, k in ((255, 5), (256, 5), (0, 6), (599, 7)):
        y[b, 1] = row(float(k), *std(1))
    return [(y0, p0), (y, p)], {"s_over3", "s_shift3", "s_beyond_256"}


def hp_at_threshold():
    """A prediction height whose IoU hp / 32 is bit-equal to one of result()'s thresholds."""
    found = [hp for hp in range(17, 33) if F(hp / 32) in thresholds()]
    assert found == [24] and thresholds()[5] == F(0.75)
    return float(found[0])


def case_result_full():
    """Three images of 14 rows, each row a label of class K and its prediction: 42 entries of
    confidence > 0.  Only 5 confidences occur, so equal ones sit in all three slots with
    IoUs between 17/32 and 1, among them 24/32, bit-equal to the threshold 0.75."""
    y, p = blank(3, 14)
    hp_at_threshold()
    for b in range(3):
        for i in range(14):
            matched(y, p, b, i, i, i, 8.0 + i, 17.0 + (3 * i + 5 * b + 7) % 16, (3 * i + b) % 5)
    assert any(v == 24 for v in p[..., 4].ravel())
    return [(y, p)], {"r_full", "r_conf_tie", "r_iou_eq_thr", "d_full", "d_hit"}


def case_result_mixed():
    """Class 10 only predicted (label quantity 0, AP 0, counted in the mean), class 11 only
    labelled, class 12 in two images with the same confidence: IoU 3/4 (the threshold) in the
    older slot and 1 in the newer one."""
    y, p = blank(2, 10)
    hp = hp_at_threshold()
    for b in range(2):
        matched(y, p, b, 0, 3, 0, 16.0, (hp, H)[b], 6, k=12)
    p[0, 0] = row(cls(10, 2), *std(8))
    p[0, 1] = row(cls(10, 1), *std(9))
    y[1, 4] = row(11.0, *std(10))
    return [(y, p)], {"r_pred_only", "r_label_only", "r_conf_tie", "r_iou_eq_thr", "c_under",
                      "b"}


def case_one_box():
    """boxes = 1: a hit, a label alone, a prediction of another class alone."""
    y, p = blank(3, 1)
    _seen(y, p, 0, 4)
    y[1, 0] = row(float(K), *std(0))
    p[2, 0] = row(cls(40, 9), *std(0))
    return [(y, p)], {"d_hit", "b", "c_under", "d_fifo_front_zero"}


# The four cases tests/test_map_kat.py derives by hand: one image of 17 rows each, class K
# alone, so the per-threshold AP is the class's AP.
def kat_c_over():
    y, p = blank(1, 17)
    image_c(p, 0, 17)
    return [(y, p)], {"c_over"}


def kat_d_full():
    y, p = blank(1, 17)
    image_d_full(y, p, 0, extras=1)
    return [(y, p)], {"d_full", "d_hit", "d_area_order"}


def kat_d_cut():
    y, p = blank(1, 17)
    image_d_cut(y, p, 0, hits=5, left=12)
    return [(y, p)], {"d_left_cut", "d_hit", "d_area_order"}


def kat_equal_areas():
    y, p = blank(1, 17)
    image_equal_areas(y, p, 0)
    return [(y, p)], {"d_area_tie", "d_area_order", "d_hit", "d_fifo_front_zero"}


def _sized(fn):
    return {"%s_%d" % (fn.__name__[5:], nb): (lambda nb=nb: fn(nb)) for nb in (15, 17, 64)}


CASES = {}
for _fn in (case_scenario_c, case_d_full, case_d_cut, case_equal_areas, case_tie_at_max):
    CASES.update(_sized(_fn))
CASES.update({
    "kat_c_over": kat_c_over, "kat_d_full": kat_d_full, "kat_d_cut": kat_d_cut,
    "kat_equal_areas": kat_equal_areas,
    "thresholds_10": case_thresholds, "one_box_1": case_one_box,
    "result_full_14": case_result_full, "result_mixed_10": case_result_mixed,
    "state_calls_3": case_state_calls, "state_600_2": case_state_600,
})


# ------------------------------------------------------------------ vtd_iou: designed pairs
_ULP = float(np.nextafter(F(32), F(0)))              # the float32 below 32
IOU_PAIRS = (                                        # name, label box, prediction box, literal
    ("touch_edge", (16, 16, 16, 16), (32, 16, 16, 16), 0.0),     # 24 < 24 is false
    ("touch_corner", (16, 16, 16, 16), (32, 32, 16, 16), 0.0),
    ("identical", BOX[2:], BOX[2:], 1.0),                          # 100 / (100 + 1e-8)
    ("overlap_one_ulp", (16, 16, 16, 16), (_ULP, 16, 16, 16), None),
    ("inside", (16, 16, 16, 16), (18, 15, 4, 8), None),
    ("zero_height", (16, 16, 0, 16), (16, 16, 16, 16), None),
    ("two_points", (16, 16, 0, 0), (16, 16, 0, 0), None),
    ("kat_064", BOX[2:], (9.5, 9.5, 8, 8), None),
    ("disjoint", (16, 16, 16, 16), (100, 100, 16, 16), None),
    ("removed_row", BOX[2:], (-8, -8, -8, -8), None),
)


def iou_operands(n, stride):
    """n rows of `stride` channels tiling IOU_PAIRS; the boxes are the last 4 channels, the
    others hold a value that would change the result if it were read."""
    lab = np.full((n, stride), 1e6, F)
    pred = np.full((n, stride), -1e6, F)
    reps = -(-n // len(IOU_PAIRS))
    lab[:, -4:] = np.tile(np.array([q[1] for q in IOU_PAIRS], F), (reps, 1))[:n]
    pred[:, -4:] = np.tile(np.array([q[2] for q in IOU_PAIRS], F), (reps, 1))[:n]
    return lab, pred
