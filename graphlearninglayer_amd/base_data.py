"""Device-resident base (labeled) sample provider for the GLL training step.

The reference's training step draws its labeled base set with

    base_images, base_labels = next(iter(base_loader))          FullySup.py:135
                                                                compare_to_mlp.py:43

where `base_loader` is a DataLoader over the whole base set (`select_base_data`,
utils.py:768-808: a CustomDataset of stacked tensors, transform=None) with
batch_size=len(dataset), shuffle=True, pin_memory=True and opt.num_workers workers
(FullySup.py:262-266, rebuilt at :278-281 when the base set is re-selected).  Every step
therefore creates a fresh iterator -- worker processes, per-sample __getitem__, collation,
pinning and an H2D copy -- to deliver the same N images in a new order: the logged step time
is DT 7.66 s of BT 8.05 s (save/.../output_record_20240718-235017.txt:14).

`DeviceBaseLoader` keeps the base images and labels resident in device memory (a few MB:
250 CIFAR images are 3 MB in HBM) and serves each draw as one on-device random permutation
(`torch.randperm` with the loader's own generator, then `index_select`), which is the
distribution the DataLoader's RandomSampler produces.  It is a drop-in for the loader at the
call site: `next(iter(provider))` yields one (images, labels) batch like the DataLoader does,
and `label_matrix()` gives the one-hot float matrix FullySup.py:153 builds for
`LaplaceLearningSparseHard.apply`.  `update()` replaces the base set when the caller
re-selects it (FullySup.py:278).

`DeviceScoreStore` is the device-resident side of that re-selection: the per-sample scores of
DatasetWithScore (utils.py:751-812) and its `select_base_data` choice as dataset indices, which
the caller gathers and hands to `DeviceBaseLoader.update`.
"""
from __future__ import annotations

import torch


class DeviceBaseLoader:
    """Whole-base-set batches from device memory, one random permutation per draw.

    data:   N x ... tensor of base samples (any dtype; images as the loader would collate them)
    labels: N integer class labels
    device: where the set lives (default: the current CUDA device, else the CPU)
    shuffle: permute every draw (the reference loader uses shuffle=True)
    seed:   seeds the loader's own generator (None: nondeterministic, like the DataLoader)
    """

    def __init__(self, data, labels, device=None, shuffle=True, seed=None, num_classes=10):
        if device is None:
            device = (torch.device("cuda", torch.cuda.current_device())
                      if torch.cuda.is_available() else torch.device("cpu"))
        self.device = torch.device(device)
        self.shuffle = bool(shuffle)
        self.num_classes = int(num_classes)
        self._gen = torch.Generator(device=self.device)
        if seed is None:
            self._gen.seed()
        else:
            self._gen.manual_seed(int(seed))
        self.update(data, labels)

    @classmethod
    def from_dataset(cls, dataset, **kw):
        """Build from a map-style dataset of (sample, label) items -- the CustomDataset that
        select_base_data returns (utils.py:806), whose .data / .labels tensors are used as they
        are when its transform is None."""
        if getattr(dataset, "transform", None) is None and hasattr(dataset, "data") \
                and hasattr(dataset, "labels"):
            data, labels = torch.as_tensor(dataset.data), torch.as_tensor(dataset.labels)
        else:
            items = [dataset[i] for i in range(len(dataset))]
            data = torch.stack([torch.as_tensor(x) for x, _ in items])
            labels = torch.as_tensor([int(y) for _, y in items])
        return cls(data, labels, **kw)

    def update(self, data, labels) -> None:
        """Replace the base set (the reference re-selects it every gl_update_base_epochs)."""
        data = torch.as_tensor(data)
        labels = torch.as_tensor(labels)
        if data.shape[0] != labels.shape[0]:
            raise ValueError(f"{data.shape[0]} samples but {labels.shape[0]} labels")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError("labels must be integer class indices")
        self.data = data.to(self.device).contiguous()
        self.labels = labels.to(self.device, torch.int64).contiguous()
        self._last_labels = None   # labels of the latest draw, in that draw's order

    def __len__(self) -> int:
        return int(self.data.shape[0])

    def sample(self):
        """One draw: (images, labels) of the whole base set in a fresh random order."""
        if not self.shuffle:
            self._last_labels = self.labels
            return self.data, self.labels
        perm = torch.randperm(len(self), device=self.device, generator=self._gen)
        lab = self.labels.index_select(0, perm)
        self._last_labels = lab
        return self.data.index_select(0, perm), lab

    def __iter__(self):
        # one batch per iterator, as DataLoader(batch_size=len(dataset)) yields
        yield self.sample()

    def label_matrix(self, labels=None) -> torch.Tensor:
        """One-hot float32 label matrix of a draw (FullySup.py:153).  Without `labels`: the
        labels of the latest draw, in that draw's order, so the rows line up with the images
        `next(iter(provider))` returned; before any draw that is an error (the stored order
        matches no batch the caller holds)."""
        if labels is None:
            if self._last_labels is None:
                raise RuntimeError("label_matrix(): no draw yet -- pass the labels of the batch")
            labels = self._last_labels
        return torch.nn.functional.one_hot(labels, num_classes=self.num_classes).float()


class DeviceScoreStore:
    """The score store and base selection of DatasetWithScore (utils.py:751-812) without the
    images: per-sample scores in device memory and `select_indices`, which returns the dataset
    indices `select_base_data` would stack -- the caller gathers its own resident data with them
    and hands the result to `DeviceBaseLoader.update(data[idx], labels[idx])`.

    labels: N integer class labels of the training set
    device: where the store lives (default: the current CUDA device, else the CPU)
    seed:   seeds the store's own generator for mode='random' (None: nondeterministic)

    `scores` (float32 zeros of shape N) is what `LaplaceLearningSparseHard.objective` takes as
    `score_out`: the layer call then writes the step's scores itself and the reference's
    per-sample `update_score` loop (FullySup.py:174-175) disappears.  The class order is the
    order of first appearance in `labels`, the insertion order of prepare_class_indices.
    """

    def __init__(self, labels, device=None, seed=None):
        if device is None:
            device = (torch.device("cuda", torch.cuda.current_device())
                      if torch.cuda.is_available() else torch.device("cpu"))
        self.device = torch.device(device)
        labels = torch.as_tensor(labels)
        if labels.dim() != 1:
            raise ValueError("labels must have shape N")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError("labels must be integer class indices")
        self.labels = labels.to(self.device, torch.int64).contiguous()
        n = self.labels.shape[0]
        self.scores = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._gen = torch.Generator(device=self.device)
        if seed is None:
            self._gen.seed()
        else:
            self._gen.manual_seed(int(seed))
        # classes by first appearance; each class's indices ascending (set-up, done once)
        uniq, inv = torch.unique(self.labels, return_inverse=True)
        first = torch.full((uniq.shape[0],), n, dtype=torch.int64, device=self.device)
        first.scatter_reduce_(0, inv, torch.arange(n, device=self.device), reduce="amin")
        self.classes = uniq[torch.argsort(first)]
        self.class_indices = [torch.nonzero(self.labels == c).flatten()
                              for c in self.classes.tolist()]

    def __len__(self) -> int:
        return int(self.scores.shape[0])

    def update_score(self, index, new_score) -> None:
        """scores[index] = new_score for a whole batch at once (utils.py:765-766 takes one
        sample per call): one index_put_, no host synchronisation for device arguments."""
        index = torch.as_tensor(index).to(self.device, torch.int64)
        new_score = torch.as_tensor(new_score).detach().to(self.device, torch.float32)
        self.scores.index_put_((index,), new_score)

    def _by_score(self, idx, count):
        """The first `count` of `idx` (ascending dataset indices) by score descending; equal
        scores keep ascending index (Python's stable sorted(..., reverse=True)); NaN after every
        number, -inf included."""
        s = self.scores.index_select(0, idx)
        nan = torch.isnan(s)
        # torch.sort ranks NaN first when descending: rank it as -inf, then move it behind -inf
        # with a second stable sort on the flag; + 0.0 makes -0.0 tie with 0.0 as Python does
        key = torch.where(nan, torch.full_like(s, float("-inf")), s) + 0.0
        order = torch.sort(key, descending=True, stable=True).indices
        order = order[torch.sort(nan[order].to(torch.uint8), stable=True).indices]
        return idx.index_select(0, order[:count])

    def _at_random(self, idx, count):
        perm = torch.randperm(idx.shape[0], device=self.device, generator=self._gen)
        return idx.index_select(0, perm[:count])

    def select_indices(self, num_samples, class_uniform_sample=False, mode="random"):
        """int64 dataset indices of the next base set (select_base_data, utils.py:768-792).
        mode='score': the highest scores; mode='random': uniform without replacement from the
        store's generator.  class_uniform_sample: num_samples // (classes present) per class --
        the whole class where it is smaller -- classes concatenated in first-appearance order."""
        if mode == "score":
            pick = self._by_score
        elif mode == "random":
            pick = self._at_random
        else:
            raise ValueError(mode)
        num_samples = int(num_samples)
        if not class_uniform_sample:
            if mode == "random" and num_samples > len(self):   # random.sample raises too
                raise ValueError("sample larger than the population")
            return pick(torch.arange(len(self), device=self.device), max(num_samples, 0))
        per_class = num_samples // max(len(self.class_indices), 1)
        parts = [pick(idx, min(per_class, idx.shape[0])) for idx in self.class_indices]
        if not parts:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        return torch.cat(parts)
