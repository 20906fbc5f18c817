"""tests/map_designs.py on the CPU: the walker equals oracle/vtd_map.py on every designed case
and on the fuzz, every case reaches the branches it declares and together they reach all of
them, every mutant is caught by some case, and the fuzz alone does not cover the list."""
import numpy as np
import pytest

from oracle import vtd_map as M
from tests import map_designs as D

_ORACLE = {}


def oracle_run(name):
    """Per-update (state, per-threshold AP, mAP) of the oracle on a designed case, computed
    once and left unchanged."""
    if name not in _ORACLE:
        ref, steps = M.MeanAveragePrecision(), []
        for y, p in D.CASES[name]()[0]:
            ref.update_state(y, p)
            steps.append((ref.latest_positive_bboxes.copy(), ref.labels_quantity_per_image.copy(),
                          ref.showed_up_classes.copy(), np.array(ref.per_iou(), np.float32),
                          ref.result()))
        _ORACLE[name] = steps
    return _ORACLE[name]


def same_as(walked, step):
    return (np.array_equal(walked.latest_positive_bboxes, step[0])
            and np.array_equal(walked.labels_quantity_per_image, step[1])
            and np.array_equal(walked.showed_up_classes, step[2])
            and np.array_equal(np.array(walked.per_iou(), np.float32), step[3]))


def walked_run(name, mutant=None):
    w = D.Walked(mutant)
    for y, p in D.CASES[name]()[0]:
        w.update_state(y, p)
    return w


def test_shapes_and_values():
    """At most 64 boxes; the sized cases at 15, 17 and 64, one case at 1 and one at 14; finite."""
    sizes = set()
    for name, fn in D.CASES.items():
        for y, p in fn()[0]:
            assert y.shape == p.shape and y.shape[2] == 6 and 1 <= y.shape[1] <= 64, name
            assert y.dtype == p.dtype == np.float32
            assert np.isfinite(y).all() and np.isfinite(p).all()
            assert str(y.shape[1]) == name.rsplit("_", 1)[1] or name.startswith("kat_"), name
            sizes.add(y.shape[1])
    assert {1, 14, 15, 17, 64} <= sizes


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_walker_equals_oracle_on_designed_case(name):
    """Every (image, class) record, then the state, the per-threshold AP and the mAP after
    every update_state."""
    w = D.Walked()
    for (y, p), step in zip(D.CASES[name]()[0], oracle_run(name)):
        for b in range(0, y.shape[0], max(1, y.shape[0] // 8)):
            for c in range(M.CLASSES):
                got, want = D.walk(y[b], p[b], c), M.image_category_record(y[b], p[b], c)
                assert got[:2] == want[:2], (name, b, c)
                assert (got[2] is None) == (want[2] is None)
                if want[2] is not None:
                    np.testing.assert_array_equal(np.array(got[2]), np.array(want[2]))
        w.update_state(y, p)
        assert same_as(w, step), name
        assert w.result() == step[4]


def test_walker_equals_oracle_on_the_fuzz():
    for run in D.fuzz_batches():
        w, ref = D.Walked(), M.MeanAveragePrecision()
        for y, p in run:
            w.update_state(y, p)
            ref.update_state(y, p)
        np.testing.assert_array_equal(w.latest_positive_bboxes, ref.latest_positive_bboxes)
        np.testing.assert_array_equal(w.labels_quantity_per_image, ref.labels_quantity_per_image)
        np.testing.assert_array_equal(w.showed_up_classes, ref.showed_up_classes)
        np.testing.assert_array_equal(np.array(w.per_iou(), np.float32),
                                      np.array(ref.per_iou(), np.float32))
        assert w.result() == ref.result()


def test_every_tag_is_reached_by_a_designed_case():
    reached = {}
    for name in sorted(D.CASES):
        w = walked_run(name)
        w.per_iou()
        declared = D.CASES[name]()[1]
        assert declared <= set(D.TAGS), name
        assert declared <= w.tags, (name, sorted(declared - w.tags))
        for t in w.tags:
            reached.setdefault(t, []).append(name)
    print("\n%-18s %s" % ("tag", "designed cases that reach it"))
    for t in D.TAGS:
        print("%-18s %s" % (t, ", ".join(reached.get(t, ())) or "-"))
    assert set(reached) == set(D.TAGS), sorted(set(D.TAGS) - set(reached))


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_every_mutant_is_caught(mutant):
    caught = []
    for name in sorted(D.CASES, key=lambda n: n == "state_600_2" and mutant != "first_256"):
        w = walked_run(name, mutant)
        if not same_as(w, oracle_run(name)[-1]):
            caught.append(name)
            if len(caught) == 3:
                break
    print("\n%s (%s): caught by %s" % (mutant, D.MUTANTS[mutant], ", ".join(caught) or "-"))
    assert caught, mutant


def test_the_fuzz_alone_does_not_cover_the_list():
    """The replay of test_map_random_batches_match_oracle and test_map_batch_larger_than_block
    (tests/test_gpu_metrics.py): what their 1951 related (image, class) records reach.  The
    sort and cut of scenario c, the 14-hit exit, the cut of the left-overs and equal areas are
    never reached, which is why the designed cases exist."""
    records, counts = D.fuzz_replay()
    print("\nfuzz replay: %d related (image, class) records" % records)
    for t in D.TAGS:
        print("%-18s %d" % (t, counts.get(t, 0)))
    assert records == 1951
    assert counts["b"] == 678 and counts["c_under"] == 370
    assert counts["d_hit"] > 0 and counts["d_tie_hit"] > 0 and counts["d_left_fit"] > 0
    for t in ("c_exact", "c_over", "d_full", "d_left_cut", "d_area_tie"):
        assert counts.get(t, 0) == 0, t
    assert not set(D.TAGS) <= set(counts)
