"""On-device task sampling: learn2learn ``TaskDataset.sample()`` for a dataset that lives in HBM.

Reference: utils/data_pre.py:16-112 builds ``l2l.data.TaskDataset(dataset, task_transforms=[FilterLabels?, NWays(ways),
KShots(2*shots), LoadData, RemapLabels, ConsecutiveLabels, RandomClassRotation?], num_tasks=...)`` and the training loop
calls ``tasks.sample()`` once per task (vision/maml_vision.py:103,116), which loads ``2*shots*ways`` images on the host and
copies them to the device.  Here the whole dataset is resident on the GPU (Mini-ImageNet train split: 0.8 GB as bytes, 3.3 GB
as fp32, of 288 GB), the host draws only the image *indices* of a meta-batch (a few KB) and one HIP launch (mi_sample_tasks)
gathers -- and for Omniglot rotates -- the pixels straight into the ``[T, 2*shots*ways, C, H, W]`` batch the engine consumes.

learn2learn is not vendored by the reference (parity unpinned at this boundary); the transform semantics restated here:
  FilterLabels(labels)      keep the samples of the given classes                      (data_pre.py:29,41,53)
  NWays(n)                  n distinct classes, uniformly
  KShots(k)                 k distinct samples of every chosen class, uniformly (replacement=False)
  RemapLabels(shuffle=True) task labels 0..n-1, assigned to the chosen classes in random order
  ConsecutiveLabels         rows grouped by class, classes in ascending ORIGINAL label order -- prepare_batch's even/odd row
                            split (data_pre.py:122-127) relies on this grouping, not on the label values
  RandomClassRotation(degs) one angle per class and task, applied to all of its images (quarter turns only)
  num_tasks=N               a task is a pure function of its id in [0, N): sampling an id twice yields the same task

``TaskSampler(..., draw='device')`` draws the indices on the device too (mi_draw_tasks): one small launch, no host
arrays, no copies, no synchronisation.  There a task is a pure function of (seed, task id) -- Philox4x32-10 keyed by the seed, counter
(id_lo, id_hi, stream, block), integer arithmetic only -- so a rank draws its own slice of the global task stream and
``describe_task(tid)`` re-derives any task on the host, bit for bit, from a logged id.  The default, ``draw='host'``, is the numpy draw.
"""
import numpy as np
import torch

from .. import _lib

_M32 = 0xffffffff
STREAM_TASK_ID, STREAM_CLASSES, STREAM_LABELS, STREAM_ROTATIONS, STREAM_SAMPLES = 0, 1, 2, 3, 16
DEVICE_DRAW_MAX_WAYS, DEVICE_DRAW_MAX_K = 32, 64          # csrc/kernels.h: kDrawMaxWays, kDrawMaxK


def philox4x32(counter, key):
    """Philox4x32-10: four 32-bit words from a four-word counter and a two-word key."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def philox_words(seed, ident, stream):
    """The 32-bit words of one stream of one id, in order: word w is output w % 4 of block w // 4; key = the 64-bit seed's halves,
    counter = (id_lo, id_hi, stream, block)."""
    key = (seed & _M32, (seed >> 32) & _M32)
    block = 0
    while True:
        yield from philox4x32((ident & _M32, (ident >> 32) & _M32, stream, block), key)
        block += 1


def bounded(words, b):
    """Exactly uniform integer in [0, b), 1 <= b < 2^32, from an iterator of 32-bit words (Lemire's multiply-and-reject)."""
    m = next(words) * b
    if (m & _M32) < b:
        t = ((1 << 32) - b) % b
        while (m & _M32) < t:
            m = next(words) * b
    return m >> 32


def select_ordered(words, k, m):
    """k out of range(m) without replacement, uniform over ORDERED k-tuples (prepare_batch splits a class's rows even/odd, so the order
    matters): Fisher-Yates on a virtual identity array, `a` holding only the overridden positions."""
    a, out = {}, []
    for i in range(k):
        j = i + bounded(words, m - i)
        out.append(a.get(j, j))
        a[j] = a.get(i, i)
    return out


class ResidentDataset:
    """images [N, C, H, W] (uint8 raw pixels or float32) and labels [N], images kept on the GPU; the label -> indices table
    of learn2learn's MetaDataset stays on the host."""

    def __init__(self, images, labels, device='cuda'):
        images = torch.as_tensor(images)
        if images.dim() != 4 or images.dtype not in (torch.uint8, torch.float32):
            raise ValueError('images must be [N, C, H, W] uint8 or float32')
        labels = np.asarray(labels).astype(np.int64).ravel()
        if labels.shape[0] != images.shape[0]:
            raise ValueError('one label per image')
        if (images.shape[1] * images.shape[2] * images.shape[3]) % 4:
            raise ValueError('C*H*W must be a multiple of 4')
        self.images = images.contiguous().to(device)
        self.labels = labels
        self.labels_to_indices = {int(c): np.nonzero(labels == c)[0] for c in np.unique(labels)}

    def __len__(self):
        return self.images.shape[0]


class TaskSampler:
    def __init__(self, dataset, ways, shots, classes=None, rotations=None, remap_shuffle=True, num_tasks=-1, seed=0, draw='host'):
        self.dataset, self.ways, self.shots = dataset, int(ways), int(shots)
        classes = sorted(dataset.labels_to_indices) if classes is None else sorted(int(c) for c in classes)
        missing = [c for c in classes if c not in dataset.labels_to_indices]
        if missing:
            raise ValueError(f'classes not in the dataset: {missing[:5]}')
        if len(classes) < self.ways:
            raise ValueError(f'{len(classes)} classes cannot form {self.ways}-way tasks')
        short = [c for c in classes if len(dataset.labels_to_indices[c]) < 2 * self.shots]
        if short:
            raise ValueError(f'classes with fewer than 2*shots = {2 * self.shots} samples: {short[:5]}')
        self.classes = np.asarray(classes, dtype=np.int64)
        if rotations is not None:
            rot = [float(r) for r in rotations]
            if any(r % 90.0 for r in rot):
                raise ValueError('only multiples of 90 degrees (the reference uses [0, 90, 180, 270], data_pre.py:34)')
            if dataset.images.shape[2] != dataset.images.shape[3]:
                raise ValueError('rotations need square images')
            rotations = np.asarray([int(r // 90) % 4 for r in rot], dtype=np.uint8)
        self.rotations = rotations
        self.remap_shuffle = bool(remap_shuffle)
        self.num_tasks = int(num_tasks)
        self.seed = int(seed)
        self._rng = np.random.default_rng([self.seed, 0x5a3])
        self._lib = None
        if draw not in ('host', 'device'):
            raise ValueError("draw must be 'host' or 'device'")
        self.draw = draw
        self.base = 0                                          # draw='device': slots handed out so far, all ranks of a call together
        self._tables = None
        if draw == 'device':
            self._init_device_draw()

    # ---------------------------------------------------------------------------------------------------- host side (indices)
    def task_description(self, rng):
        """(image index [n2], task label [n2], quarter turns [n2] or None) of one task drawn from `rng`."""
        k = 2 * self.shots
        chosen = np.sort(rng.choice(self.classes, size=self.ways, replace=False))          # NWays; ConsecutiveLabels order
        new_label = rng.permutation(self.ways) if self.remap_shuffle else np.arange(self.ways)   # RemapLabels
        index = np.concatenate([rng.choice(self.dataset.labels_to_indices[int(c)], size=k, replace=False) for c in chosen])
        labels = np.repeat(new_label.astype(np.int64), k)
        rot = None
        if self.rotations is not None:
            rot = np.repeat(rng.choice(self.rotations, size=self.ways), k).astype(np.uint8)   # one angle per class
        return index.astype(np.int64), labels, rot

    def sample_indices(self, tasks):
        """Indices of `tasks` tasks: (index [T, n2] int64, labels [T, n2] int64, rot [T, n2] uint8 or None), host arrays."""
        out = []
        for _ in range(tasks):
            if self.num_tasks > 0:
                tid = int(self._rng.integers(self.num_tasks))
                out.append(self.task_description(np.random.default_rng([self.seed, 0x7a5c, tid])))
            else:
                out.append(self.task_description(self._rng))
        index = np.stack([o[0] for o in out])
        labels = np.stack([o[1] for o in out])
        rot = np.stack([o[2] for o in out]) if self.rotations is not None else None
        return index, labels, rot

    # ------------------------------------------------------------------------------------------ counter-based draw
    def _draw_tables(self):
        """(class_offsets [nC + 1], class_index) int32 on the host: class c of the eligible classes (ascending label) owns the ascending
        image ids class_index[class_offsets[c] : class_offsets[c + 1]]."""
        if self._tables is None:
            lists = [np.sort(self.dataset.labels_to_indices[int(c)]) for c in self.classes]
            self._tables = (np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32),
                            np.concatenate(lists).astype(np.int32))
        return self._tables

    def _init_device_draw(self):
        k, ds = 2 * self.shots, self.dataset.images
        if not ds.is_cuda:
            raise RuntimeError("draw='device' draws on the GPU (mi_draw_tasks); the dataset must be resident there")
        if self.ways > DEVICE_DRAW_MAX_WAYS or k > DEVICE_DRAW_MAX_K:
            raise ValueError(f"draw='device' supports ways <= {DEVICE_DRAW_MAX_WAYS} and 2*shots <= {DEVICE_DRAW_MAX_K}")
        if len(self.dataset) >= 2 ** 31:
            raise ValueError("draw='device' keeps image ids as int32: the dataset must hold fewer than 2^31 images")
        if not 0 <= self.seed < 2 ** 64 or self.num_tasks >= 2 ** 32 or (self.rotations is not None and len(self.rotations) > 256):
            raise ValueError("draw='device' takes a seed in [0, 2^64), num_tasks < 2^32 and at most 256 rotations")
        offsets, index = self._draw_tables()
        self._offsets_d = torch.from_numpy(offsets).to(ds.device)
        self._index_d = torch.from_numpy(index).to(ds.device)
        self._rot_d = torch.from_numpy(self.rotations).to(ds.device) if self.rotations is not None else None

    def task_ids(self, first_slot, tasks):
        """Task ids (uint64 [tasks]) of slots first_slot .. first_slot + tasks - 1: the slot itself, or with num_tasks = N > 0 a uniform
        pick in [0, N) from stream 0 of the slot.  Host arithmetic on (seed, num_tasks) alone."""
        slots = [(int(first_slot) + t) & (2 ** 64 - 1) for t in range(tasks)]
        if self.num_tasks > 0:
            slots = [bounded(philox_words(self.seed, s, STREAM_TASK_ID), self.num_tasks) for s in slots]
        return np.asarray(slots, dtype=np.uint64)

    def describe_task(self, tid):
        """(image index [n2] int64, task label [n2] int64, quarter turns [n2] uint8 or None) of task `tid`, host arrays: the numpy
        restatement of mi_draw_tasks, equal to it bit for bit.  A pure function of (seed, tid) that needs no GPU: it re-derives a
        task of a draw='device' sampler from a logged id (and says nothing about the numpy stream of draw='host')."""
        tid, k = int(tid), 2 * self.shots
        off, class_index = self._draw_tables()
        chosen = sorted(select_ordered(philox_words(self.seed, tid, STREAM_CLASSES), self.ways, len(self.classes)))
        new_label = (select_ordered(philox_words(self.seed, tid, STREAM_LABELS), self.ways, self.ways) if self.remap_shuffle
                     else range(self.ways))
        index = np.concatenate([class_index[off[c] + np.asarray(select_ordered(philox_words(self.seed, tid, STREAM_SAMPLES + j),
                                                                                      k, int(off[c + 1] - off[c])), dtype=np.int64)]
                                for j, c in enumerate(chosen)])
        labels = np.repeat(np.asarray(new_label, dtype=np.int64), k)
        rot = None
        if self.rotations is not None:
            words = philox_words(self.seed, tid, STREAM_ROTATIONS)
            rot = np.repeat(np.asarray([self.rotations[bounded(words, len(self.rotations))] for _ in range(self.ways)], dtype=np.uint8), k)
        return index.astype(np.int64), labels, rot

    def draw_device(self, tasks, rank=0, world=1):
        """Draw `tasks` tasks with one launch on the current stream: device tensors (index [T, n2] int64, labels [T, n2] int64,
        rot [T, n2] uint8 or None, task ids [T] int64 holding the uint64 bit pattern).  Rank r of `world` takes slots
        base + r*tasks .. base + (r+1)*tasks - 1 and every rank advances base by world*tasks, so the ranks of a call draw disjoint
        slices of one global task stream without talking to each other.  Nothing here reads device memory or waits for the device."""
        import ctypes as C
        if self.draw != 'device':
            raise RuntimeError("this sampler draws on the host; build it with draw='device'")
        tasks, rank, world = int(tasks), int(rank), int(world)
        if tasks < 1 or not 0 <= rank < world:
            raise ValueError('tasks >= 1 and 0 <= rank < world')
        if self._lib is None:
            self._lib = _lib.load()
        dev, n2 = self.dataset.images.device, 2 * self.shots * self.ways
        index = torch.empty((tasks, n2), dtype=torch.int64, device=dev)
        labels = torch.empty((tasks, n2), dtype=torch.int64, device=dev)
        rot = torch.empty((tasks, n2), dtype=torch.uint8, device=dev) if self._rot_d is not None else None
        ids = torch.empty((tasks,), dtype=torch.int64, device=dev)
        first_slot = (self.base + rank * tasks) & (2 ** 64 - 1)
        rc = self._lib.mi_draw_tasks(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(self._offsets_d.data_ptr()),
                                     C.c_void_p(self._index_d.data_ptr()), len(self.classes), self.ways, 2 * self.shots,
                                     C.c_void_p(self._rot_d.data_ptr() if rot is not None else 0),
                                     len(self.rotations) if rot is not None else 0, int(self.remap_shuffle), self.seed, first_slot,
                                     max(self.num_tasks, 0), tasks, C.c_void_p(index.data_ptr()), C.c_void_p(labels.data_ptr()),
                                     C.c_void_p(rot.data_ptr() if rot is not None else 0), C.c_void_p(ids.data_ptr()))
        _lib.check(rc)
        self.base += world * tasks
        return index, labels, rot, ids

    # -------------------------------------------------------------------------------------------------- device side (pixels)
    def gather(self, index, rot=None):
        """data [T, n2, C, H, W] fp32 on the dataset's device from host index / rotation arrays (mi_sample_tasks)."""
        ds = self.dataset.images
        if not ds.is_cuda:
            raise RuntimeError('the task sampler gathers on the GPU (mi_sample_tasks); the dataset must be resident there')
        index = np.ascontiguousarray(index, dtype=np.int64)
        if index.min() < 0 or index.max() >= len(self.dataset):
            raise IndexError('image index out of range')
        idx_d = torch.from_numpy(index).to(ds.device)
        rot_d = torch.from_numpy(np.ascontiguousarray(rot, dtype=np.uint8)).to(ds.device) if rot is not None else None
        return self._gather_device(idx_d, rot_d)

    def _gather_device(self, idx_d, rot_d):
        """mi_sample_tasks on device tensors index [T, n2] int64 / rot [T, n2] uint8 or None; the caller guarantees the index range."""
        import ctypes as C
        if self._lib is None:
            self._lib = _lib.load()
        ds = self.dataset.images
        T, n2 = idx_d.shape
        out = torch.empty((T, n2) + tuple(ds.shape[1:]), dtype=torch.float32, device=ds.device)
        rc = self._lib.mi_sample_tasks(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(ds.data_ptr()),
                                       int(ds.dtype == torch.uint8), len(self.dataset), ds.shape[1], ds.shape[2], ds.shape[3],
                                       C.c_void_p(idx_d.data_ptr()), C.c_void_p(rot_d.data_ptr() if rot_d is not None else 0),
                                       T, n2, C.c_void_p(out.data_ptr()))
        _lib.check(rc)
        return out

    def sample_batch(self, tasks, rank=0, world=1):
        """A meta-batch: (data [T, 2*shots*ways, C, H, W] fp32, labels [T, 2*shots*ways] int64), both on the GPU.  With draw='device'
        two launches on the current stream (mi_draw_tasks, mi_sample_tasks) and nothing else; `rank` / `world` as in draw_device."""
        if self.draw == 'device':
            index, labels, rot, _ = self.draw_device(tasks, rank, world)
            return self._gather_device(index, rot), labels
        if (rank, world) != (0, 1):
            raise ValueError("rank slices of one task stream need draw='device' (the host rng is a sequential stream)")
        index, labels, rot = self.sample_indices(tasks)
        return self.gather(index, rot), torch.from_numpy(labels).to(self.dataset.images.device)

    def sample(self):
        """One task, the return value of learn2learn's ``tasks.sample()``: (data [n2, C, H, W], labels [n2])."""
        data, labels = self.sample_batch(1)
        return data[0], labels[0]
