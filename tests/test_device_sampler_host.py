"""The counter-based task draw on the host: Philox4x32-10 known answers, Lemire's bounded integer on hand-made
words, and the numpy mirror TaskSampler.describe_task / task_ids -- structure, determinism and uniformity.  The GPU kernel is compared
with this mirror bit for bit in test_gpu_device_sampler.py.  Reference path: utils/data_pre.py:16-112."""
import numpy as np
import pytest
import torch

from exploring_meta_amd.utils import synthetic
from exploring_meta_amd.utils import task_sampler as TS
from exploring_meta_amd.utils.task_sampler import ResidentDataset, TaskSampler
from oracle import sampler_ref as S

# 0.999 quantiles of the chi-square distribution (standard tables)
CHI2_999 = {3: 16.266, 4: 18.467, 11: 31.264}


def _dataset(n_classes, per_class, c=1, hw=8):
    n = n_classes * per_class
    imgs = synthetic.hash_uniform(91, (n, c, hw, hw)).astype(np.float32)
    labels = np.repeat(np.arange(n_classes) * 3 + 7, per_class)        # non-contiguous original labels
    perm = np.argsort(synthetic.hash_uniform(5, (n,)))                   # interleave the classes
    return labels[perm], ResidentDataset(torch.from_numpy(imgs[perm]), labels[perm], device='cpu')


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(counter, key, want):
    assert ' '.join(f'{w:08x}' for w in TS.philox4x32(counter, key)) == want


def test_philox_words_walk_the_blocks_of_one_stream():
    seed, ident, stream = 0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e
    words = TS.philox_words(seed, ident, stream)
    got = [next(words) for _ in range(9)]
    key, ctr = (0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e)
    assert got == [w for b in range(3) for w in TS.philox4x32(ctr + (b,), key)][:9]


def test_bounded_on_hand_made_words():
    words = iter([0, 0x80000000, 7])
    assert TS.bounded(words, 3) == 1                     # word 0: l = 0 < 2^32 % 3 = 1, rejected; word 2^31: m = 3 * 2^31, m >> 32 = 1
    assert next(words) == 7                              # exactly two words consumed
    words = iter([0xdeadbeef, 7])
    assert TS.bounded(words, 1) == 0 and next(words) == 7               # b = 1: one word, result 0
    words = iter([2, 7])
    assert TS.bounded(words, 3) == 0 and next(words) == 7               # l = 6 >= b: accepted without computing the threshold
    # a bound above 2^31: b = 3 * 2^30, threshold t = 2^32 % b = 2^30
    b = 3 << 30
    words = iter([1, 0x40000000, 0xffffffff, 7])
    # word 1: m = b, l = b mod 2^32 = b >= t -> accepted, result 0
    assert TS.bounded(words, b) == 0 and next(words) == 0x40000000
    # word 2^30 + 1: m = 3 * 2^60 + b, l = b -> accepted, m >> 32 = 3 * 2^28
    assert TS.bounded(iter([0x40000001]), b) == 3 << 28
    # word 4: m = 3 * 2^32, l = 0 < t -> rejected; word 2^32 - 1: m = b * 2^32 - b, l = 2^32 - b = 2^30 >= t -> accepted, b - 1
    words = iter([4, 0xffffffff, 7])
    assert TS.bounded(words, b) == b - 1 and next(words) == 7


def test_select_ordered_is_a_fisher_yates_prefix():
    for seed in range(20):
        full = TS.select_ordered(TS.philox_words(seed, 1, 2), 9, 9)
        assert sorted(full) == list(range(9))                            # k == m: a permutation
        part = TS.select_ordered(TS.philox_words(seed, 1, 2), 4, 9)
        assert part == full[:4]                                          # the first k steps of the same shuffle
    assert TS.select_ordered(iter([1, 1, 1]), 3, 3) == [0, 1, 2]         # bounded gives 0, so j = i every time
    # j = 2, then j = 1 + 1 = 2 again: the second step must see the override a[2] = a[0] = 0
    assert TS.select_ordered(iter([0xffffffff, 0xffffffff, 0]), 3, 3) == [2, 0, 1]


@pytest.mark.parametrize('ways,shots,rotations,shuffle', [(5, 1, None, True), (5, 5, None, False), (20, 1, [0.0, 90.0, 180.0, 270.0], True)])
def test_mirror_task_structure(ways, shots, rotations, shuffle):
    labels, ds = _dataset(30, 12)
    classes = sorted(set(labels.tolist()))[:25]
    sm = TaskSampler(ds, ways, shots, classes=classes, rotations=rotations, remap_shuffle=shuffle, seed=3)
    tasks = [sm.describe_task(t) for t in sm.task_ids(0, 16)]
    for index, lab, rot in tasks:
        assert index.dtype == np.int64 and lab.dtype == np.int64 and (rot is None) == (rotations is None)
        S.check_task_structure(index, lab, rot, labels, ways, shots, classes)
        if not shuffle:
            assert (lab == np.repeat(np.arange(ways), 2 * shots)).all()
        if rot is not None:
            assert rot.dtype == np.uint8 and set(rot.tolist()) <= {0, 1, 2, 3}
    assert len({tuple(t[0].tolist()) for t in tasks}) > 1                # tasks differ


def test_describe_task_is_a_pure_function_of_seed_and_id():
    labels, ds = _dataset(10, 6)
    a = TaskSampler(ds, 5, 1, rotations=[0.0, 90.0], seed=(5 << 32) + 1)
    b = TaskSampler(ds, 5, 1, rotations=[0.0, 90.0], seed=(5 << 32) + 1)
    ids = [0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 11]
    fwd = [a.describe_task(t) for t in ids]
    bwd = [b.describe_task(t) for t in reversed(ids)][::-1]              # another order, another sampler object
    for x, y in zip(fwd, bwd):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert not np.array_equal(fwd[3][0], fwd[4][0])                      # the id's high word is part of the counter
    other = TaskSampler(ds, 5, 1, rotations=[0.0, 90.0], seed=1).describe_task(0)
    assert not np.array_equal(other[0], fwd[0][0])                       # and the seed's high word part of the key
    assert a.task_ids(2 ** 32 - 2, 4).tolist() == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]


def test_num_tasks_makes_tasks_a_function_of_their_id():
    labels, ds = _dataset(10, 6)
    sm = TaskSampler(ds, 5, 1, num_tasks=3, seed=1)
    ids = sm.task_ids(0, 40)
    assert ids.dtype == np.uint64 and set(ids.tolist()) <= {0, 1, 2}
    assert np.array_equal(ids[7:19], sm.task_ids(7, 12))                 # a slot's id does not depend on the slice it is asked in
    seen = {}
    for t in ids.tolist():
        index, lab, _ = sm.describe_task(t)
        row = tuple(index.tolist()) + tuple(lab.tolist())
        assert seen.setdefault(t, row) == row                            # each of the <= 3 tasks always identical
    assert len(set(seen.values())) == len(seen) <= 3


def test_device_draw_needs_a_resident_dataset():
    labels, ds = _dataset(10, 6)
    with pytest.raises(RuntimeError):
        TaskSampler(ds, 5, 1, draw='device')                              # a CPU dataset
    with pytest.raises(ValueError):
        TaskSampler(ds, 5, 1, draw='gpu')
    with pytest.raises(RuntimeError):
        TaskSampler(ds, 5, 1).draw_device(2)                              # a host-draw sampler has no device tables


# ---------------------------------------------------------------------------------------------------------------- uniformity
# Fixed seeds, so these are deterministic.  Each statistic is chi-square distributed under the hypothesis that the draw is uniform
# and is held below the 0.999 quantile of its degrees of freedom.

def _chi2(counts, expected):
    counts = np.asarray(counts, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


def test_uniform_class_appearances():
    """5 of 12 classes over n = 4000 tasks.  The 12 appearance counts are not multinomial: every task adds exactly 5, so a count is
    Binomial(n, p = 5/12) and two counts are negatively correlated.  With p2 = (5*4)/(12*11) the chance that two given classes
    appear together, the covariance matrix is n c (I - J/12) with c = p (1 - p) - (p2 - p^2) = 35/132, so sum (O - n p)^2 / (n c) is
    chi-square with 11 degrees of freedom (dividing by n p instead would shrink the statistic by c / p = 0.64 and weaken the test)."""
    labels, ds = _dataset(12, 4)
    sm = TaskSampler(ds, 5, 1, seed=101)
    n, counts = 4000, np.zeros(12)
    classes = sorted(set(labels.tolist()))
    for t in range(n):
        index, _, _ = sm.describe_task(t)
        for c in set(labels[index].tolist()):
            counts[classes.index(c)] += 1
    assert counts.sum() == 5 * n
    p, p2 = 5 / 12, 20 / 132
    c = p * (1 - p) - (p2 - p * p)
    stat = float(((counts - n * p) ** 2).sum() / (n * c))
    print('class appearances: chi2(11) =', stat)
    assert stat < CHI2_999[11]


def test_uniform_ordered_sample_pairs():
    """The ORDERED pair (first, second sample) of a class with m = 4 images, k = 2: 12 equally likely cells, 11 degrees of freedom.
    A subset-only algorithm (Floyd's without a shuffle) puts all its mass on part of the cells and fails this."""
    labels, ds = _dataset(5, 4)
    sm = TaskSampler(ds, 5, 1, seed=202)
    first = int(sorted(set(labels.tolist()))[0])
    where = {int(i): p for p, i in enumerate(np.sort(np.nonzero(labels == first)[0]))}   # image id -> position in the class
    n, counts = 6000, np.zeros((4, 4))
    for t in range(n):
        index, _, _ = sm.describe_task(t)
        counts[where[int(index[0])], where[int(index[1])]] += 1           # ways == n_classes: the first class is always chosen
    assert np.trace(counts) == 0
    stat = _chi2(counts[~np.eye(4, dtype=bool)], n / 12)
    print('ordered sample pairs: chi2(11) =', stat)
    assert stat < CHI2_999[11]


def test_uniform_label_of_the_first_class():
    labels, ds = _dataset(12, 4)
    sm = TaskSampler(ds, 5, 1, seed=303)
    n, counts = 4000, np.zeros(5)
    for t in range(n):
        counts[sm.describe_task(t)[1][0]] += 1
    stat = _chi2(counts, n / 5)
    print('label of the first class: chi2(4) =', stat)
    assert stat < CHI2_999[4]


def test_uniform_rotation_of_the_first_class():
    labels, ds = _dataset(12, 4)
    sm = TaskSampler(ds, 5, 1, rotations=[0.0, 90.0, 180.0, 270.0], seed=404)
    n, counts = 4000, np.zeros(4)
    for t in range(n):
        counts[sm.describe_task(t)[2][0]] += 1
    stat = _chi2(counts, n / 4)
    print('rotation of the first class: chi2(3) =', stat)
    assert stat < CHI2_999[3]


def test_abi_rejects_unsupported_shapes_before_any_launch():
    """mi_draw_tasks checks its shape arguments on the host: beyond ways <= 32 / k <= 64 it returns an error status and a text, and
    touches no device (this runs without one; the pointers are never dereferenced)."""
    import ctypes as C
    from exploring_meta_amd import _lib
    lib = _lib.load()
    ptr = C.c_void_p(64)

    def call(n_classes, ways, k, n_rot=0, num_tasks=0, tasks=1):
        return lib.mi_draw_tasks(None, ptr, ptr, n_classes, ways, k, ptr if n_rot else None, n_rot, 1, 1, 0, num_tasks, tasks, ptr, ptr,
                                 ptr if n_rot else None, None)
    for args in [(40, 33, 2), (40, 5, 65), (40, 5, 0), (4, 5, 2), (40, 0, 2), (40, 5, 2, 257), (40, 5, 2, 0, 2 ** 32), (40, 5, 2, 0, 0, 0)]:
        assert call(*args) != 0, args
        assert b'mi_draw_tasks' in lib.mi_last_error(None)
    with pytest.raises(_lib.MiError):
        _lib.check(call(40, 33, 2))


# ---- the inputs of the limit tests (tests/test_gpu_device_sampler.py), checked on the mirror

@pytest.mark.parametrize('num_tasks,seed,slots', S.REJECTION_DRAWS)
def test_large_bounds_reject_often_enough_to_test_the_loop(num_tasks, seed, slots):
    """At least 8 of the 64 slots consume more than one word for the id draw (expected: 32 and 16), the recount agrees with
    task_ids, and the first word of a rejecting slot is indeed below the threshold 2^32 mod b."""
    assert num_tasks in (2 ** 31 + 1, 3 * 2 ** 30) and slots == 64
    labels, ds = _dataset(10, 6)
    sm = TaskSampler(ds, 5, 1, num_tasks=num_tasks, seed=seed)
    draws = [S.id_draw_words(seed, slot, num_tasks) for slot in range(slots)]
    assert sm.task_ids(0, slots).tolist() == [d[0] for d in draws] and all(0 <= d[0] < num_tasks for d in draws)
    rejecting = [slot for slot, d in enumerate(draws) if d[1] > 1]
    print(f'num_tasks {num_tasks}: {len(rejecting)} of {slots} slots reject, at most {max(d[1] for d in draws)} words')
    assert len(rejecting) >= 8
    t = (2 ** 32 - num_tasks) % num_tasks
    for slot in range(slots):
        first = next(TS.philox_words(seed, slot, TS.STREAM_TASK_ID))
        assert ((first * num_tasks) & 0xffffffff < t) == (slot in rejecting)


def test_python_surface_admits_256_rotations_and_full_tables():
    labels, ds = _dataset(30, 12)
    rotations = [90.0 * (i & 3) for i in range(256)]
    sm = TaskSampler(ds, 20, 1, rotations=rotations, seed=13)
    assert sm.rotations.dtype == np.uint8 and sm.rotations.tolist() == [i & 3 for i in range(256)]
    index, lab, rot = sm.describe_task(5)
    words = TS.philox_words(13, 5, TS.STREAM_ROTATIONS)
    assert rot[::2].tolist() == [TS.bounded(words, 256) & 3 for _ in range(20)]
    # ways = 32, k = 64 on 34 classes of 64..70 images
    sizes = [64 + (3 * c) % 7 for c in range(34)]
    lab34 = np.repeat(np.arange(34) * 3 + 7, sizes)
    ds34 = ResidentDataset(torch.zeros(len(lab34), 1, 2, 2), lab34, device='cpu')
    big = TaskSampler(ds34, 32, 32, rotations=[0.0, 90.0, 180.0, 270.0], seed=6)
    index, lab, rot = big.describe_task(1)
    S.check_task_structure(index, lab, rot, lab34, 32, 32, big.classes.tolist())
