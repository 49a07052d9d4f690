"""The counter-based task draw on the GPU (csrc/sampler.hip, mi_draw_tasks) against its numpy mirror
TaskSampler.describe_task / task_ids, bit for bit, and the sampled batch against oracle/sampler_ref.py.
Reference path: utils/data_pre.py:16-112 + tasks.sample() (vision/maml_vision.py:103,116)."""
import numpy as np
import pytest
import torch

from exploring_meta_amd.utils import synthetic
from exploring_meta_amd.utils.task_sampler import ResidentDataset, TaskSampler
from oracle import sampler_ref as S
from gpu_utils import report

pytestmark = pytest.mark.gpu


def _dataset(sizes, c=1, hw=8, dtype='f32'):
    """One class per entry of `sizes` (images per class), non-contiguous original labels, classes interleaved."""
    n = int(np.sum(sizes))
    u = synthetic.hash_uniform(91, (n, c, hw, hw))
    imgs = (u * 256).astype(np.uint8) if dtype == 'u8' else u.astype(np.float32)
    labels = np.repeat(np.arange(len(sizes)) * 3 + 7, sizes)
    perm = np.argsort(synthetic.hash_uniform(5, (n,)))
    return imgs[perm], labels[perm], ResidentDataset(torch.from_numpy(imgs[perm]), labels[perm], device='cuda')


def _mirror(sm, first_slot, tasks):
    ids = sm.task_ids(first_slot, tasks)
    rows = [sm.describe_task(t) for t in ids.tolist()]
    rot = np.stack([r[2] for r in rows]) if sm.rotations is not None else None
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), rot, ids


def _assert_draw_equals_mirror(sm, tasks, rank=0, world=1):
    first = sm.base + rank * tasks
    index, labels, rot, ids = sm.draw_device(tasks, rank, world)
    assert index.is_cuda and index.dtype == torch.int64 and labels.dtype == torch.int64 and ids.dtype == torch.int64
    windex, wlabels, wrot, wids = _mirror(sm, first, tasks)
    assert np.array_equal(ids.cpu().numpy().view(np.uint64), wids)
    assert np.array_equal(index.cpu().numpy(), windex)
    assert np.array_equal(labels.cpu().numpy(), wlabels)
    assert (rot is None) == (wrot is None)
    if rot is not None:
        assert rot.dtype == torch.uint8 and np.array_equal(rot.cpu().numpy(), wrot)
    return windex, wlabels, wrot, wids


CASES = {
    '5w1s': dict(sizes=[6] * 10, ways=5, shots=1),
    '5w5s_unshuffled_unequal': dict(sizes=list(range(10, 24)), ways=5, shots=5, remap_shuffle=False),
    '20w1s_rot_subset': dict(sizes=[12] * 30, ways=20, shots=1, rotations=[0.0, 90.0, 180.0, 270.0], subset=25),
    'full_permutations': dict(sizes=[4] * 6, ways=6, shots=2, rotations=[90.0, 270.0]),           # ways == n_classes, k == m
    'ways_cap': dict(sizes=[3] * 34, ways=32, shots=1),
    'k_cap': dict(sizes=[70, 64, 66], ways=2, shots=32),                                            # k = 64, one class with k == m
}


def _sampler(name, **kw):
    case = dict(CASES[name])
    imgs, labels, ds = _dataset(case.pop('sizes'))
    subset = case.pop('subset', None)
    classes = sorted(set(labels.tolist()))[:subset] if subset else None
    return labels, TaskSampler(ds, classes=classes, draw='device', **case, **kw)


@pytest.mark.parametrize('name', list(CASES))
def test_draw_bit_exact_against_the_mirror(name):
    labels, sm = _sampler(name, seed=3)
    for tasks in (1, 3, 67):                                              # one block, a few, more blocks than a small grid
        windex, wlabels, wrot, _ = _assert_draw_equals_mirror(sm, tasks)
    assert sm.base == 71
    case = CASES[name]
    for t in range(0, 67, 11):
        S.check_task_structure(windex[t], wlabels[t], None if wrot is None else wrot[t], labels, case['ways'], case['shots'],
                               sm.classes.tolist())
    assert len({tuple(r) for r in windex.tolist()}) > 1


def test_seed_and_slot_use_all_64_bits():
    labels, sm = _sampler('20w1s_rot_subset', seed=(0x9e37 << 32) + 5)   # a seed above 2^32: the key's second word
    _assert_draw_equals_mirror(sm, 3)
    low = _sampler('20w1s_rot_subset', seed=5)[1].draw_device(3)
    sm.base = 0
    assert not torch.equal(sm.draw_device(3)[0], low[0])
    sm.base = 2 ** 32 - 2                                                 # the slot counter's high word changes inside one launch
    _, _, _, wids = _assert_draw_equals_mirror(sm, 5)
    assert wids.tolist() == [2 ** 32 - 2 + t for t in range(5)] and sm.base == 2 ** 32 + 3
    sm.base = 2 ** 63 + 7                                                 # ids above the int64 range keep their bit pattern
    _assert_draw_equals_mirror(sm, 2)


@pytest.mark.parametrize('num_tasks', [-1, 5])
def test_a_task_does_not_depend_on_its_batch(num_tasks):
    whole = _sampler('20w1s_rot_subset', seed=8, num_tasks=num_tasks)[1].draw_device(67)
    parts = _sampler('20w1s_rot_subset', seed=8, num_tasks=num_tasks)[1]
    pieces = [parts.draw_device(n) for n in (1, 2, 64)]
    for w, *p in zip(whole, *pieces):
        assert torch.equal(w, torch.cat(p))


def test_rank_slices_of_one_task_stream():
    full = _sampler('20w1s_rot_subset', seed=4)[1]
    r0, r1 = _sampler('20w1s_rot_subset', seed=4)[1], _sampler('20w1s_rot_subset', seed=4)[1]
    for step in range(2):
        whole = full.draw_device(8)
        a, b = r0.draw_device(4, rank=0, world=2), r1.draw_device(4, rank=1, world=2)
        for w, x, y in zip(whole, a, b):
            assert torch.equal(w, torch.cat([x, y]))
        assert r0.base == r1.base == full.base == 8 * (step + 1)


def test_num_tasks_mode():
    labels, sm = _sampler('5w1s', seed=1, num_tasks=3)
    windex, wlabels, _, wids = _assert_draw_equals_mirror(sm, 40)
    assert set(wids.tolist()) <= {0, 1, 2}
    assert len({tuple(a) + tuple(b) for a, b in zip(windex.tolist(), wlabels.tolist())}) == len(set(wids.tolist()))


@pytest.mark.parametrize('dtype,c,hw,rotations', [('u8', 3, 84, None), ('f32', 1, 28, [0.0, 90.0, 180.0, 270.0])])
def test_sampled_pixels_bit_exact(dtype, c, hw, rotations):
    imgs, labels, ds = _dataset([8] * 12, c, hw, dtype)
    sm = TaskSampler(ds, 5, 2, rotations=rotations, seed=9, draw='device')
    data, lab = sm.sample_batch(6)
    windex, wlabels, wrot, _ = _mirror(sm, 0, 6)
    want = S.gather_tasks(imgs, windex, wrot)
    got = data.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
    assert lab.is_cuda and lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), wlabels)
    if rotations is not None:
        assert len(set(wrot.ravel().tolist())) > 1
    one, one_lab = sm.sample()                                            # slot 6
    w1 = _mirror(sm, 6, 1)
    assert sm.base == 7 and np.array_equal(one.cpu().numpy(), S.gather_tasks(imgs, w1[0], w1[2])[0])
    assert np.array_equal(one_lab.cpu().numpy(), w1[1][0])


def test_device_drawn_batch_feeds_the_engine():
    """tasks.sample() -> the batched engine entry (maml_vision.py:103-112) with indices and pixels both drawn on the device."""
    from exploring_meta_amd import core_functions as cf
    ways, shots = 5, 1
    n_cls, per = 8, 4
    protos = synthetic.hash_uniform(3, (n_cls, 1, 28, 28))
    noise = synthetic.hash_uniform(4, (n_cls, per, 1, 28, 28))
    imgs = ((protos[:, None] > 0.5) ^ (noise > 0.9)).astype(np.float32).reshape(n_cls * per, 1, 28, 28)
    ds = ResidentDataset(torch.from_numpy(imgs), np.repeat(np.arange(n_cls), per))
    sm = TaskSampler(ds, ways, shots, rotations=[0.0, 90.0, 180.0, 270.0], seed=2, draw='device')
    torch.manual_seed(0)
    maml = cf.MAML(cf.OmniglotCNN(ways).cuda(), lr=0.5, first_order=False)
    data, lab = sm.sample_batch(4)
    assert data.shape == (4, 2 * shots * ways, 1, 28, 28) and data.is_cuda and lab.dtype == torch.int64
    total, losses, accs = cf.meta_batch_adapt(maml.clone(), data, lab, 1, shots, ways)
    assert losses.shape == (4,) and torch.isfinite(losses).all()


def test_argument_errors():
    imgs, labels, ds = _dataset([2] * 34)
    with pytest.raises(ValueError):
        TaskSampler(ds, 33, 1, draw='device')                              # ways above the cap: raised on the host, nothing launched
    TaskSampler(ds, 33, 1)                                                 # (the host draw has no cap)
    imgs, labels, ds = _dataset([66] * 3)
    with pytest.raises(ValueError):
        TaskSampler(ds, 2, 33, draw='device')                              # k = 66 above the cap
    cpu = ResidentDataset(torch.from_numpy(imgs), labels, device='cpu')
    with pytest.raises(RuntimeError):
        TaskSampler(cpu, 2, 1, draw='device')
    sm = TaskSampler(ds, 2, 1, draw='device')
    with pytest.raises(ValueError):
        sm.draw_device(0)
    with pytest.raises(ValueError):
        sm.draw_device(2, rank=2, world=2)
    with pytest.raises(ValueError):
        TaskSampler(ds, 2, 1).sample_batch(2, rank=1, world=2)             # rank slices need the counter-based draw
    assert sm.base == 0


# ------------------------------------------------------------------------------------------ the limits of the stated domain
# mi_maml.h: ways <= 32, k <= 64, n_rot <= 256, num_tasks < 2^32

@pytest.mark.parametrize('num_tasks,seed,slots', S.REJECTION_DRAWS)
def test_id_draw_with_a_bound_above_2_31_runs_the_rejection_loop(num_tasks, seed, slots):
    """Philox::bounded's `while (l < t)`: with num_tasks = 2^31 + 1 / 3 * 2^30 a word is rejected with probability 1/2 / 1/4 (the host
    test counts the slots that do), so the device loop runs; ids, indices, labels and rotations equal the mirror."""
    labels, sm = _sampler('20w1s_rot_subset', seed=seed, num_tasks=num_tasks)
    rejecting = sum(S.id_draw_words(seed, slot, num_tasks)[1] > 1 for slot in range(slots))
    assert rejecting >= 8
    windex, wlabels, wrot, wids = _assert_draw_equals_mirror(sm, slots)
    assert wids.tolist() == [S.id_draw_words(seed, slot, num_tasks)[0] for slot in range(slots)]
    assert len(set(wids.tolist())) == slots and int(wids.max()) >= 2 ** 30 and wrot is not None
    report(f'draw_rejection[{num_tasks}]', slots_rejecting=rejecting, mismatches=0)


def test_every_table_full_32_ways_of_64_rows():
    """ways = 32 with k = 64: every LDS table of the kernel full (2048 rows per task, 64 override entries per lane), rotations on."""
    sizes = [64 + (3 * c) % 7 for c in range(34)]
    assert min(sizes) == 64 and max(sizes) == 70
    imgs, labels, ds = _dataset(sizes)
    sm = TaskSampler(ds, 32, 32, rotations=[0.0, 90.0, 180.0, 270.0], seed=6, draw='device')
    windex, wlabels, wrot, _ = _assert_draw_equals_mirror(sm, 3)
    assert windex.shape == (3, 2048)
    for t in range(3):
        S.check_task_structure(windex[t], wlabels[t], wrot[t], labels, 32, 32, sm.classes.tolist())
    assert len(set(wrot.ravel().tolist())) == 4
    report('draw_32_ways_64_rows', mismatches=0)


def test_rotation_table_at_its_cap():
    """n_rot = 256: the rotation stream is stream 3 with bounded(256); the table entry i is i & 3, so a row's turns are the low bits of
    the entry the draw picked."""
    imgs, labels, ds = _dataset([12] * 30)
    rotations = [90.0 * (i & 3) for i in range(256)]
    sm = TaskSampler(ds, 20, 1, rotations=rotations, seed=13, draw='device')
    assert sm.rotations.tolist() == [i & 3 for i in range(256)]
    windex, wlabels, wrot, wids = _assert_draw_equals_mirror(sm, 40)
    from exploring_meta_amd.utils import task_sampler as TS
    for t in (0, 17, 39):
        words = TS.philox_words(13, int(wids[t]), TS.STREAM_ROTATIONS)
        assert wrot[t, ::2].tolist() == [TS.bounded(words, 256) & 3 for _ in range(20)]
    assert len(set(wrot.ravel().tolist())) == 4
    with pytest.raises(ValueError):
        TaskSampler(ds, 20, 1, rotations=rotations + [0.0], draw='device')
    report('draw_256_rotations', mismatches=0)
