"""Host-side data utilities of the DMVAE drop-in -- the counterpart of the parts of
code/includes/utils.py that the hot path touches: sample_gumbel (:17-19),
get_clustering_accuracy (:22-34), load_data("mnist") (:122-148) and Dataset
(:428-466), and for the mixture-of-experts models the label generators (:37-74)
and MEDataset (:378-425).  The other loaders are out of scope."""
import gzip
import math
import os
import struct
import types

import numpy as np


def sample_gumbel(shape, eps=1e-20):
    """includes/utils.py:17-19 (same global NumPy RNG, same formula)."""
    U = np.random.uniform(0, 1, shape)
    return -np.log(eps - np.log(U + eps))


def accuracy_from_confusion(d, size):
    """The Hungarian step of includes/utils.py:28-34 on a confusion matrix d[cluster][class] (square, integer counts) of `size`
    rows: the best one-to-one assignment of clusters to classes; scipy's solver replaces the removed
    sklearn.utils.linear_assignment_.  Shared by the host evaluation (below) and the device one, which builds d on the GPU."""
    from scipy.optimize import linear_sum_assignment
    d = np.asarray(d, dtype=np.int64)
    r, c = linear_sum_assignment(d.max() - d)
    return d[r, c].sum() / (size * 1.0)


def get_clustering_accuracy(weights, classes):
    """includes/utils.py:22-34."""
    clusters = np.argmax(weights, axis=-1)
    n_classes = weights.shape[1]
    size = len(clusters)
    d = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(d, (clusters, np.asarray(classes, dtype=np.int64)), 1)
    return accuracy_from_confusion(d, size)


def synthetic_images(n, dim=784, seed=0, density=0.19):
    """Deterministic MNIST-like stand-in used when no idx files are present and
    by the benchmark: x = u * 1[v < density], u, v ~ U[0,1)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, dim), dtype=np.float32)
    v = rng.random((n, dim), dtype=np.float32)
    return (u * (v < density)).astype(np.float32)


def _read_idx(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        magic, = struct.unpack(">I", f.read(4))
        nd = magic & 0xFF
        dims = struct.unpack(">" + "I" * nd, f.read(4 * nd))
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(dims)


def _find(root, stem):
    for ext in ("", ".gz"):
        for sep in ("-", "."):
            p = os.path.join(root, stem.replace("-idx", sep + "idx") + ext)
            if os.path.exists(p):
                return p
    return None


def load_data(datagroup, **args):
    """load_data("mnist") of the reference (includes/utils.py:77,122-148): float
    grey levels in [0,1] used as soft Bernoulli targets, NOT binarised (SURVEY
    F6); TF's 55 000 / 10 000 train/test split.  Reads idx files from
    data/<datagroup>/ when present; otherwise (no network in this image) a
    deterministic synthetic stand-in of the same shapes, flagged in
    dataset.synthetic."""
    if datagroup not in ("mnist", "fashion-mnist", "synthetic"):
        raise NotImplementedError("dataset %r: only the MNIST-shaped DMVAE path is built (SURVEY.md 2.1)" % datagroup)
    ds = types.SimpleNamespace(datagroup=datagroup, input_dim=784, input_type="binary", n_classes=10,
                               sample_plot=None, regeneration_plot=None, synthetic=False)
    root = os.path.join(os.environ.get("DMVAE_DATA", "data"), datagroup)
    ti = _find(root, "train-images-idx3-ubyte") if datagroup != "synthetic" else None
    if ti:
        tl, si, sl = (_find(root, s) for s in ("train-labels-idx1-ubyte", "t10k-images-idx3-ubyte", "t10k-labels-idx1-ubyte"))
        tr = _read_idx(ti).reshape(-1, 784).astype(np.float32) / 255.0
        te = _read_idx(si).reshape(-1, 784).astype(np.float32) / 255.0
        ds.train_data, ds.train_classes = tr[:55000], _read_idx(tl)[:55000].astype(np.int64)
        ds.test_data, ds.test_classes = te, _read_idx(sl).astype(np.int64)
    else:
        ds.synthetic = True
        n_tr, n_te = int(args.get("n_train", 55000)), int(args.get("n_test", 10000))
        allx = synthetic_images(n_tr + n_te, 784, seed=0)
        cls = np.random.RandomState(0).randint(0, 10, n_tr + n_te)
        ds.train_data, ds.train_classes = allx[:n_tr], cls[:n_tr]
        ds.test_data, ds.test_classes = allx[n_tr:], cls[n_tr:]
    ds.train_labels = ds.test_labels = None
    if args.get("moe"):
        # train.py:146-151 of the reference (MoE models only: the regression labels draw from the global NumPy stream): one-hot
        # classes, or the regression targets of a random linear expert per class
        if args.get("classification"):
            ds.train_labels, ds.test_labels = generate_classification_variables(ds)
        else:
            ds.train_labels, ds.test_labels = generate_regression_variable(ds, int(args["output_dim"]))
    return ds


def generate_regression_variable(dataset, output_dim):
    """includes/utils.py:37-59: one random linear expert per class of the dataset, drawn from the global NumPy stream (biases
    [O, E_d] first, then weights [O, I, E_d]); the label of a row is its own class's expert applied to it."""
    n_experts = dataset.n_classes
    input_dim = dataset.train_data.shape[1]
    biases = np.random.randn(output_dim, n_experts)
    weights = np.random.randn(output_dim, input_dim, n_experts)

    def labels(X, cls):
        out = np.empty((len(X), output_dim))
        for e in range(n_experts):          # (row by class: the reference's [N, O, E_d] tensor is never formed)
            rows = np.nonzero(np.asarray(cls) == e)[0]
            out[rows] = X[rows].astype(np.float64) @ weights[:, :, e].T + biases[:, e]
        return out
    return labels(dataset.train_data, dataset.train_classes), labels(dataset.test_data, dataset.test_classes)


def generate_classification_variables(dataset):
    """includes/utils.py:62-74: one-hot over the dataset's classes"""
    eye = np.eye(dataset.n_classes)
    return eye[np.asarray(dataset.train_classes, dtype=np.int64)], eye[np.asarray(dataset.test_classes, dtype=np.int64)]


def get_moe_clustering_accuracy(weights, classes, n_classes):
    """get_clustering_accuracy for the mixture-of-experts models.  DEVIATION from the reference, which calls
    get_clustering_accuracy (includes/utils.py:22-34) and sizes its confusion matrix by the number of EXPERTS: with fewer experts
    than classes (the CLI default, 5 experts on 10 MNIST classes) it raises IndexError at the first evaluation.  Here the matrix is
    max(E, n_classes) square and the rectangular assignment is solved by scipy's Hungarian solver."""
    clusters = np.argmax(weights, axis=-1)
    n = max(weights.shape[1], int(n_classes), int(np.max(classes)) + 1 if len(classes) else 0)
    d = np.zeros((n, n), dtype=np.int64)
    np.add.at(d, (clusters, np.asarray(classes, dtype=np.int64)), 1)
    return accuracy_from_confusion(d, len(clusters))


def _device_classes(ds, device):
    """the unpermuted int32 classes of a data set, resident next to device_rows (uploaded once)"""
    import torch
    key = "classes:" + str(device)
    if key not in ds._device:
        ds._device[key] = torch.as_tensor(np.ascontiguousarray(ds._cls, dtype=np.int32)).to(device)
    return ds._device[key]


BINARIZE_MODES = ("off", "static", "dynamic", "threshold")


def choose_labeled(classes, n_labeled, n_classes, seed, rows=None):
    """Stratified choice of the rows that keep their label (semi-supervised training): class c gets
    n_labeled // n_classes rows, the remainder goes to the lowest classes one each.  The draw is per class, in ascending class order, from
    np.random.RandomState(seed): the global NumPy stream is never touched, so a run shuffles and samples as it did.  rows: draw among
    these row indices only (train.py: the train split's).  Returns the sorted int64 row indices; a class with fewer rows than its quota
    raises ValueError."""
    classes = np.asarray(classes)
    n_labeled, n_classes = int(n_labeled), int(n_classes)
    if n_labeled < 0 or n_classes < 1:
        raise ValueError("choose_labeled: n_labeled = %d, n_classes = %d" % (n_labeled, n_classes))
    pool = np.arange(len(classes)) if rows is None else np.asarray(rows, dtype=np.int64)
    rng = np.random.RandomState(int(seed))
    picked = []
    for c in range(n_classes):
        quota = n_labeled // n_classes + (1 if c < n_labeled % n_classes else 0)
        mine = pool[classes[pool] == c]
        if len(mine) < quota:
            raise ValueError("choose_labeled: class %d has %d rows, its quota is %d" % (c, len(mine), quota))
        picked.append(np.sort(mine[rng.permutation(len(mine))[:quota]]))
    return np.sort(np.concatenate(picked)).astype(np.int64) if picked else np.zeros(0, dtype=np.int64)


class Dataset:
    """includes/utils.py:428-466.  Same contract: shuffle on construction and at
    every get_batches() with the global NumPy RNG, consecutive batches, short
    last batch.  Instead of physically permuting the rows each epoch the class
    keeps the cumulative row order; `data` / `classes` present the permuted
    view, and the device-resident copy is gathered by that order on the GPU
    (dmvae_gather_rows).

    binarize ("off" = the reference, grey levels as soft targets): "static" one Bernoulli draw of the rows, "dynamic" a
    fresh draw per epoch -- the draw counter is the number of reshuffle() calls so far --, "threshold" x > 0.5.  The draw is made on the
    device (dmvae_hip.binarize) into a second resident buffer that device_rows returns in place of the grey rows; binarize_seed keys it, and
    the ranks of a data-parallel run pass the same one: they hold the whole data set and must agree on it.  No NumPy draw is consumed.

    augment (None = off): a dmvae_hip.augment.AugmentSpec or its string.  train_rows(device) then returns a further
    resident buffer with every grey row warped by its own random affine map, redrawn per epoch like the "dynamic" draw (counter = reshuffle()
    calls so far, keyed by augment_seed, the same on every rank) and, with binarize != "off", binarised after the warp.  device_rows, data,
    get_batches and the labels stay the clean rows."""

    def __init__(self, data, batch_size=100, shuffle=True, binarize="off", binarize_seed=0, labeled=None, augment=None, augment_seed=0):
        data, classes = data
        if binarize not in BINARIZE_MODES:
            raise ValueError("binarize = %r: one of %s" % (binarize, ", ".join(BINARIZE_MODES)))
        self._rows = np.ascontiguousarray(np.asarray(data, dtype=np.float32))
        self._cls = np.copy(classes)
        # labeled: indices (choose_labeled) of the UNPERMUTED rows whose class a semi-supervised model may see; a reshuffle moves nothing
        self.labeled = None if labeled is None else np.unique(np.asarray(labeled, dtype=np.int64))
        if self.labeled is not None and len(self.labeled) and (self.labeled[0] < 0 or self.labeled[-1] >= len(self._rows)):
            raise ValueError("Dataset: labeled row indices outside [0, %d)" % len(self._rows))
        self.order = np.arange(len(self._rows))
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.data_dim = self._rows.shape[1]
        self.epoch_len = int(math.ceil(len(self._rows) / batch_size))
        self._device = {}
        self.binarize = binarize
        self.binarize_seed = int(binarize_seed)
        self._reshuffles = 0                   # reshuffle() calls so far: the draw counter of "dynamic"
        self._draws = {}                       # device -> the counter of the draw its binarised buffer holds
        self._host_draw = None                 # (counter, rows): the current draw, read back once
        self.augment = None
        self.augment_seed = int(augment_seed)
        self._train_draws = {}                 # device -> (augment counter, binarise counter) of the draw its training buffer holds
        if augment is not None:
            from dmvae_hip.augment import parse_augment
            self.augment = parse_augment(augment)
            self.augment.shape_for(self.data_dim)              # (refuses rows that are no H x W image before anything is uploaded)
        if shuffle:
            self.order = self.order[np.random.permutation(len(self._rows))]

    @property
    def data(self):
        return self._host_rows()[self.order]

    @property
    def classes(self):
        return self._cls[self.order]

    def reshuffle(self):
        """the per-epoch shuffle of get_batches (utils.py:450-454); returns the new row order"""
        self._reshuffles += 1
        if self.shuffle:
            self.order = self.order[np.random.permutation(len(self._rows))]
        return self.order

    def get_batches(self):
        order = self.reshuffle()
        rows = self._host_rows()
        for s in range(0, len(order), self.batch_size):
            yield rows[order[s:s + self.batch_size]]

    def device_rows(self, device):
        """the unpermuted rows, resident in HBM (uploaded once); binarised: the current draw of them, in a second buffer whose address never
        changes (redrawn in place, on the current stream, when its draw counter is stale)"""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.as_tensor(self._rows).to(device)
        if self.binarize == "off":
            return self._device[key]
        return self._binarized_rows(device)

    def train_rows(self, device):
        """the rows an epoch trains on: device_rows(device) itself without augmentation; with it, a resident buffer of its own whose address
        never changes, holding the warp of the GREY rows under counter draw_counter_augment() -- then binarised, in the data set's mode, seed
        and counter, when binarize != "off" -- redrawn in place on the current stream when stale"""
        if self.augment is None:
            return self.device_rows(device)
        return self._augmented_rows(device)

    def draw_counter_augment(self):
        """the Philox counter of the current augmentation draw: reshuffle() calls so far"""
        return self._reshuffles

    def _augmented_rows(self, device):
        import torch
        from dmvae_hip.augment import augment
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.as_tensor(self._rows).to(device)
        grey = self._device[key]
        if "augmented:" + key not in self._device:
            self._device["augmented:" + key] = torch.empty_like(grey)
            if self.binarize != "off":
                self._device["train:" + key] = torch.empty_like(grey)
        warped = self._device["augmented:" + key]
        want = (self.draw_counter_augment(), self.draw_counter())
        if self.binarize == "off":
            if self._train_draws.get(key) != want:
                augment(grey, self.augment, seed=self.augment_seed, counter=want[0], out=warped)
                self._train_draws[key] = want
            return warped
        from dmvae_hip.binarize import binarize
        out = self._device["train:" + key]
        if self._train_draws.get(key) != want:
            augment(grey, self.augment, seed=self.augment_seed, counter=want[0], out=warped)
            binarize(warped, seed=self.binarize_seed, counter=want[1], mode="threshold" if self.binarize == "threshold" else "bernoulli", out=out)
            self._train_draws[key] = want
        return out

    def draw_counter(self):
        """the Philox counter of the current draw: reshuffle() calls so far under "dynamic", 0 otherwise"""
        return self._reshuffles if self.binarize == "dynamic" else 0

    def _binarized_rows(self, device):
        import torch
        from dmvae_hip.binarize import binarize
        key = str(device)
        if key not in self._draws:
            self._device["binarized:" + key] = torch.empty_like(self._device[key])
        out, counter = self._device["binarized:" + key], self.draw_counter()
        if self._draws.get(key, (None, None))[1] != counter:
            binarize(self._device[key], seed=self.binarize_seed, counter=counter, mode="threshold" if self.binarize == "threshold" else "bernoulli", out=out)
            self._draws[key] = (device, counter)
        return out

    def _host_rows(self):
        """the rows the host views present: the grey rows, or the current draw read back from the device (once per draw)"""
        if self.binarize == "off":
            return self._rows
        counter = self.draw_counter()
        if self._host_draw is None or self._host_draw[0] != counter:
            if not self._draws:
                raise RuntimeError("Dataset(binarize=%r): no device draw exists yet -- the rows are binarised by the HIP kernel on the device (there "
                                   "is no CPU fallback); call device_rows(device) first" % self.binarize)
            device = next(iter(self._draws.values()))[0]
            self._host_draw = (counter, self.device_rows(device).cpu().numpy())
        return self._host_draw[1]

    def device_classes(self, device):
        return _device_classes(self, device)

    @property
    def n_labeled(self):
        return 0 if self.labeled is None else int(len(self.labeled))

    def host_labels(self):
        """int32 [N] in the unpermuted row order: the class at the labeled rows, -1 elsewhere"""
        y = np.full(len(self._rows), -1, dtype=np.int32)
        if self.n_labeled:
            y[self.labeled] = np.asarray(self._cls)[self.labeled].astype(np.int32)
        return y

    def device_labels(self, device):
        """host_labels() resident next to device_rows (uploaded once)"""
        import torch
        key = "labels:" + str(device)
        if key not in self._device:
            self._device[key] = torch.as_tensor(self.host_labels()).to(device)
        return self._device[key]

    def __len__(self):
        return self.epoch_len


class MEDataset:
    """includes/utils.py:378-425: (data, classes, labels); NO shuffle at construction, one np.random.permutation per
    get_batches() (when shuffle), consecutive batches of (X, labels, classes), short last batch.  As Dataset, the rows are not
    moved: the cumulative row order is kept, and the device copies of the rows and labels are gathered by it on the GPU."""

    def __init__(self, data, batch_size=100, shuffle=True):
        data, classes, labels = data
        self._rows = np.ascontiguousarray(np.asarray(data, dtype=np.float32))
        self._cls = np.copy(classes)
        self._lbl = np.ascontiguousarray(np.asarray(labels, dtype=np.float32))
        self.len = len(self._rows)
        assert len(self._lbl) == self.len and len(self._cls) == self.len
        self.order = np.arange(self.len)
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.data_dim = self._rows.shape[1]
        self.epoch_len = int(math.ceil(self.len / batch_size))
        self._device = {}

    @property
    def data(self):
        return self._rows[self.order]

    @property
    def classes(self):
        return self._cls[self.order]

    @property
    def labels(self):
        return self._lbl[self.order]

    def reshuffle(self):
        if self.shuffle:
            self.order = self.order[np.random.permutation(self.len)]
        return self.order

    def get_batches(self):
        order = self.reshuffle()
        for s in range(0, self.len, self.batch_size):
            o = order[s:s + self.batch_size]
            yield self._rows[o], self._lbl[o], self._cls[o]

    def device_rows(self, device):
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.as_tensor(self._rows).to(device)
        return self._device[key]

    def device_classes(self, device):
        return _device_classes(self, device)

    def device_labels(self, device):
        import torch
        key = "labels:" + str(device)
        if key not in self._device:
            self._device[key] = torch.as_tensor(self._lbl).to(device)
        return self._device[key]

    def __len__(self):
        return self.epoch_len
