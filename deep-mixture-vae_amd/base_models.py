"""VAE / DeepMixtureVAE -- drop-in for the class surface of code/base_models.py
(:14-147 VAE, :150-432 DeepMixtureVAE) with the per-batch path executed by the
MI355X HIP library (dmvae_hip) instead of a TensorFlow session.

Same constructor arguments, method names, argument order and return types:
    DeepMixtureVAE(name, input_type, input_dim, latent_dim, n_classes,
                   activation=None, initializer=None, cnn=False).build_graph()
    .define_train_step(init_lr, decay_steps, decay_rate=0.9)
    .train_op(session, data, kl_ratio=1.0) -> float      (epoch-mean loss)
    .get_accuracy(session, data) -> float
    .sample_reparametrization_variables(n, variables=None) -> dict
    .sample_generative_feed(n, **kwargs) -> dict
`session` is a dmvae_hip.Session (device / stream / rank) or None.  What were
graph tensors to fetch (mean, log_var, logits, cluster_probs, Z, decoded_X,
reconstructed_X) are methods evaluating on demand: encode(X), decode(Z),
reconstruct(X, epsilon=None).  Extensions are keyword-only and default to the
reference's behaviour: batch_size (reference hard-codes 100, train.py:215-216),
dtype ("bf16" throughput / "fp32" parity), enc_layers / head_dim / dec_layers
(reference literals 500,500 / 2000 / 2000,500,500), gumbel + temperature
(Gumbel-Softmax relaxed KL; default off = the live graph),
noise ("device" Philox | "host" NumPy stream of the reference), seed,
gmm ("host": pretrain_prior fits the prior tables' mixture with sklearn like
the reference | "device": dmvae_hip.gmm.DiagGMM, a function of (Z, seed)),
gmm_seeding (with gmm="device": "host" k-means++ in NumPy on a host copy of the
encoder means | "device": dmvae_gmm_seed on the resident means),
eval ("host": get_accuracy copies every batch's scores back and takes arg-max and
confusion matrix in NumPy | "device": both on the GPU from the resident rows, one
small matrix read back per call).
"""
import math
import os
import zipfile

import numpy as np

import priors
from includes.network import DeepNetwork
from includes.utils import accuracy_from_confusion, get_clustering_accuracy


class VAE:
    def __init__(self, name, input_type, input_dim, latent_dim, activation=None, initializer=None):
        self.name = name
        self.input_dim = input_dim
        self.latent_dim = latent_dim
        self.input_type = input_type
        self.activation = activation
        self.initializer = initializer
        self.path = ""
        self.kl_ratio = 1.0          # placeholder_with_default(1.0), base_models.py:28-30
        self.is_training = True      # placeholder_with_default(True), :32-34 (no BN on the path: unused)
        self.X = None
        self.decoded_X = None
        self.train_step = None
        self.latent_variables = dict()

    def build_graph(self, encoder_layer_sizes, decoder_layer_sizes):
        raise NotImplementedError

    def sample_reparametrization_variables(self, n, variables=None):
        """base_models.py:44-56: {epsilon placeholder name: host noise}; draws in
        the dict order of latent_variables (C then Z) from the global NumPy RNG."""
        samples = dict()
        if variables is None:
            for lv, eps, _ in self.latent_variables.values():
                if eps is not None:
                    samples[eps] = lv.sample_reparametrization_variable(n)
        else:
            for var in variables:
                lv, eps, _ = self.latent_variables[var]
                if eps is not None:
                    samples[eps] = lv.sample_reparametrization_variable(n)
        return samples

    def sample_generative_feed(self, n, **kwargs):
        samples = dict()
        for name, (lv, _, _) in self.latent_variables.items():
            kwargs_ = dict() if name not in kwargs else kwargs[name]
            samples[name] = lv.sample_generative_feed(n, **kwargs_)
        return samples

    # the three loss definitions exist as graph-building steps in the reference
    # (:66-93); here the loss is computed inside the fused step, nothing to build
    def define_latent_loss(self):
        self.latent_loss = "KL_C + KL_Z (dmvae_latent_fwd)"

    def define_recon_loss(self):
        if self.input_type not in ("binary", "real"):
            raise NotImplementedError
        self.recon_loss = "reconstruction loss (DMVAE_EPI_BIAS_RECON)"

    def define_train_loss(self):
        self.define_latent_loss()
        self.define_recon_loss()
        self.loss = "recon + kl_ratio * latent"

    def define_train_step(self, init_lr, decay_steps, decay_rate=0.9):
        """base_models.py:95-110.  exponential_decay is called with a literal
        global_step=0, so the learning rate is the constant init_lr;
        decay_steps / decay_rate are accepted and, as in the reference, inert."""
        self.define_train_loss()
        self._lr = float(init_lr)
        self._engine.write_state(lr=self._lr)
        self.train_step = "adam_tf"

    def debug(self, session, data):
        import pdb
        for batch in data.get_batches():
            feed = {"X": batch}
            feed.update(self.sample_reparametrization_variables(len(batch)))
            pdb.set_trace()
            break


def _cnn_encoder_network(out_dim):
    """the convolutional encoder as the reference specifies it (base_models.py:179-205 with ("fc", 2048 -> 500) for DMVAE,
    :459-488 with ("fc", 2048 -> 128) for VaDE): the DeepNetwork spec list drives the plan's CNN trunk -- the plan implements
    exactly this stack, any other list is refused here rather than silently ignored"""
    from dmvae_hip.runtime import CONV_STACK, CONV_FLAT
    enc_spec = [("cn", {"n_kernels": 32, "prev_n_kernels": 1, "kernel": (3, 3)}),
                ("cn", {"n_kernels": 32, "prev_n_kernels": 32, "kernel": (3, 3)}), ("mp", {"k": 2}),
                ("cn", {"n_kernels": 64, "prev_n_kernels": 32, "kernel": (3, 3)}),
                ("cn", {"n_kernels": 64, "prev_n_kernels": 64, "kernel": (3, 3)}), ("mp", {"k": 2}),
                ("cn", {"n_kernels": 128, "prev_n_kernels": 64, "kernel": (3, 3)}),
                ("cn", {"n_kernels": 128, "prev_n_kernels": 128, "kernel": (3, 3)}), ("mp", {"k": 2}),
                ("fc", {"input_dim": 2048, "output_dim": out_dim})]
    net = DeepNetwork("layers", enc_spec, activation="relu", initializer="xavier")
    stack, side = net.conv_stack(28)
    if stack != tuple((ci, co, hw, pool) for _, ci, co, hw, pool in CONV_STACK) or side * side * stack[-1][1] != CONV_FLAT:
        raise NotImplementedError("the plan's CNN trunk is the stack of base_models.py:181-202; got %r" % (stack,))
    assert net.widths() == (out_dim,)
    return net


class DeepMixtureVAE(VAE):
    def __init__(self, name, input_type, input_dim, latent_dim, n_classes, activation=None, initializer=None,
                 cnn=False, *, batch_size=100, dtype="bf16", enc_layers=(500, 500), head_dim=2000,
                 dec_layers=(2000, 500, 500), gumbel=False, temperature=1.0, noise="device", seed=0,
                 deterministic=True, session=None, gmm="host", eval="host", gmm_seeding="host", label_weight=None):
        VAE.__init__(self, name, input_type, input_dim, latent_dim, activation=activation, initializer=initializer)
        self.n_classes = n_classes
        # semi-supervised training: None = no attachment, today's plan; a number alpha attaches the cross-entropy on
        # q(c|x) of the labelled rows (csrc/label_xent.hip) at weight alpha * N / n_labeled
        self.label_weight = None if label_weight is None else float(label_weight)
        self._labels_key = None
        if gmm not in ("host", "device"):
            raise ValueError("gmm must be 'host' or 'device'")
        self.gmm = gmm
        if gmm_seeding not in ("host", "device"):
            raise ValueError("gmm_seeding must be 'host' or 'device'")
        self.gmm_seeding = gmm_seeding       # takes effect with gmm="device" only
        if eval not in ("host", "device"):
            raise ValueError("eval must be 'host' or 'device'")
        self.eval = eval
        self._eval_perm = None
        self._eval_calls = 0
        # The checked-in reference forces cnn = True (base_models.py:156); the path BASELINE.json names is
        # the MLP branch (:218-226), the default here.  cnn=True builds the checked-in trunk
        # (:176-216): six 3x3 SAME convolutions, three 2x2 SAME max-pools, FullyConnected 2048 -> 500.
        self.cnn = bool(cnn)
        if activation not in (None, "relu") and getattr(activation, "__name__", "") != "relu":
            raise NotImplementedError("activation must be ReLU (train.py:196 passes tf.nn.relu)")
        if noise not in ("device", "host"):
            raise ValueError("noise must be 'device' or 'host'")
        self.batch_size = int(batch_size)
        self.dtype = dtype
        self.enc_layers, self.head_dim, self.dec_layers = tuple(enc_layers), int(head_dim), tuple(dec_layers)
        if self.cnn:
            if int(input_dim) != 784:
                raise ValueError("cnn=True reshapes the inputs to 28x28x1 (base_models.py:176): input_dim must be 784")
            self.enc_layers = (self.enc_layers[-1],)      # the trunk's one dense layer: ("fc", 2048 -> 500), :202
        self.gumbel, self.temperature = bool(gumbel), float(temperature)
        self.noise, self.seed, self.deterministic = noise, int(seed), bool(deterministic)
        self._session = session
        self._engine = None
        self._replay = None
        self._replay_key = None
        self._perm = None

    # ------------------------------------------------------------------ graph
    def build_graph(self):
        from dmvae_hip import StepEngine, default_session
        sess = self._session or default_session()
        self._session = sess
        # decoder spec exactly as the reference writes it (base_models.py:280-288)
        prev, spec = self.latent_dim, []
        for w in self.dec_layers:
            spec.append(("fc", {"input_dim": prev, "output_dim": w}))
            prev = w
        self.decoder_network = DeepNetwork("layers", spec, activation="relu", initializer="xavier")
        assert self.decoder_network.widths() == self.dec_layers
        if self.cnn:
            self.encoder_network = _cnn_encoder_network(self.enc_layers[0])
        self._engine = StepEngine(self.input_dim, self.latent_dim, self.n_classes, enc_layers=self.enc_layers,
                                  head_dim=self.head_dim, dec_layers=self.dec_layers, input_type=self.input_type,
                                  dtype=self.dtype, max_batch=self.batch_size, mode="relaxed" if self.gumbel else "exact",
                                  temperature=self.temperature, seed=self.seed + 7919 * sess.rank,
                                  deterministic=self.deterministic, session=sess, cnn=self.cnn,
                                  moe=getattr(self, "_moe_spec", None),     # (set by models.MoE: the experts' head on this gate)
                                  labels=self._label_placeholder(sess))
        self._engine.init_parameters(self.seed)
        # names of the graph's placeholders / tensors (fetch through the methods below)
        self.X, self.epsilon, self.cluster = "X", "epsilon_Z", "epsilon_C"
        self.mean, self.log_var, self.logits = "mean", "log_var", "logits"
        self.cluster_probs, self.Z = "cluster_probs", "Z"
        self.decoded_X, self.reconstructed_X = "decoded_X", "reconstructed_X"
        self.latent_variables = dict()
        self.latent_variables.update({
            "C": (priors.DiscreteFactorial("cluster", 1, self.n_classes), self.cluster, {"logits": self.logits}),
            "Z": (priors.NormalMixtureFactorial("representation", self.latent_dim, self.n_classes, engine=self._engine),
                  self.epsilon,
                  {"mean": self.mean, "log_var": self.log_var, "weights": self.cluster_probs,
                   "cluster_sample": self.gumbel}),
        })
        return self

    @property
    def engine(self):
        return self._engine

    # ------------------------------------------------------------------ training
    def _label_placeholder(self, sess):
        """the label array a plan is attached with before a data set is known: one row without a label (_bind_labels replaces it)"""
        if self.label_weight is None:
            return None
        import torch
        return torch.full((1,), -1, dtype=torch.int32, device=sess.device)

    def _bind_labels(self, sess, data, train):
        """attached plans only: the data set's label array and the term's weight for the steps that follow -- alpha * N / n_labeled in
        train_op (over an epoch the term then estimates alpha * the mean cross-entropy of the labelled set, whatever the batch size),
        0 in the pretraining stages.  Returns the labels' device pointer (part of train_op's recapture key)."""
        if self.label_weight is None:
            return None
        if sess.world_size > 1:
            raise NotImplementedError("label_weight: the label term is built and tested on one rank")
        eng = self._engine
        if train:
            if data.labeled is None or data.n_labeled == 0:
                raise ValueError("label_weight = %g needs a data set with labeled rows (Dataset(..., labeled=choose_labeled(...)))" % self.label_weight)
            worst = int(np.max(np.asarray(data._cls)[data.labeled]))
            if worst >= self.n_classes or int(np.min(np.asarray(data._cls)[data.labeled])) < 0:
                raise ValueError("label_weight: a labeled row's class lies outside [0, n_classes = %d)" % self.n_classes)
        labels = data.device_labels(sess.device)
        key = (labels.data_ptr(), int(labels.shape[0]))
        if self._labels_key != key:
            eng.set_labels(labels)
            self._labels_key = key
        n_rows = int(labels.shape[0])
        eng.set_label_weight(self.label_weight * n_rows / data.n_labeled if train else 0.0)
        return labels.data_ptr()

    def _epoch_perm(self, data, sess):
        """the epoch's row order -> this rank's slice of every global batch, on the device.
        Returns (perm, n_full, tail, epoch_weight) -- see dmvae_hip.parallel.epoch_plan: with more than
        one rank only the full global batches are trained, the step count is the same on every rank."""
        import torch
        from dmvae_hip.parallel import epoch_plan
        order, n_full, tail, weight = epoch_plan(data.reshuffle(), data.batch_size, sess.rank, sess.world_size)
        t = torch.as_tensor(np.ascontiguousarray(order, dtype=np.int32))
        if self._perm is None or self._perm.numel() != t.numel():
            self._perm = torch.empty(t.numel(), dtype=torch.int32, device=sess.device)
        self._perm.copy_(t)
        return self._perm, n_full, tail, weight

    def train_op(self, session, data, kl_ratio=1.0):
        """One epoch, base_models.py:112-132: for every batch of data.get_batches()
        run [loss, train_step]; return sum(batch_loss) / epoch_len.  The loss is
        accumulated on the device and read back once per epoch."""
        assert(self.train_step is not None)
        import torch
        from dmvae_hip import make_exchange
        sess = session or self._session
        eng = self._engine
        world = sess.world_size
        gb = data.batch_size                                  # global batch
        if gb % world:
            raise ValueError("batch_size %d is not divisible by the world size %d" % (gb, world))
        b = gb // world                                       # per-rank batch
        if b != eng.max_batch:
            raise ValueError("per-rank batch %d != the size the model was built for (%d)" % (b, eng.max_batch))
        rows = data.train_rows(sess.device)                    # (device_rows itself unless the data set augments: DESIGN.md section 30)
        labels_ptr = self._bind_labels(sess, data, train=True)
        perm, n_full, tail, weight = self._epoch_perm(data, sess)
        import time
        torch.cuda.synchronize(sess.device)
        self._epoch_t0 = time.perf_counter()                   # (behind the row upload and the epoch's permutation: the steps themselves)
        ex = make_exchange(4 * eng.param.numel())
        sync = ex if ex.enabled else None
        eng.reset_epoch(n_full + (1 if tail else 0), kl_ratio=kl_ratio, epoch_weight=weight)
        host_noise = self.noise == "host"
        if host_noise and world > 1:
            raise NotImplementedError("noise='host' replays the reference's single-process NumPy stream; use noise='device' with more than one rank")

        def host_feed(n):
            feed = self.sample_reparametrization_variables(n)        # C (gumbel) first, then Z: reference order
            eps = torch.as_tensor(np.ascontiguousarray(feed[self.epsilon], dtype=np.float32)).to(sess.device)
            g = None
            if self.gumbel:
                g = torch.as_tensor(np.ascontiguousarray(feed[self.cluster].reshape(n, self.n_classes), dtype=np.float32)).to(sess.device)
            return eps, g

        if host_noise:
            if labels_ptr is not None:
                eng.zero_label_acc()
            for i in range(n_full):
                eps, g = host_feed(b)
                eng.train_step(rows, perm, b, eps, g, first=i * b, grad_sync=sync, grad_scale=ex.grad_scale)
        else:
            # the captured graph holds the device pointers of the rows and of the row order: recapture
            # when either buffer (another Dataset, a re-upload) or the exchange changes
            key = (rows.data_ptr(), perm.data_ptr(), b, sync is None) + (() if labels_ptr is None else (labels_ptr,))
            if n_full > 0 and (self._replay is None or self._replay_key != key):
                self._replay = eng.capture_step(rows, perm, grad_sync=sync, grad_scale=ex.grad_scale)
                self._replay_key = key
                eng.reset_epoch(n_full + (1 if tail else 0), kl_ratio=kl_ratio, epoch_weight=weight)
            if labels_ptr is not None:
                eng.zero_label_acc()                          # (behind the capture, whose warm-up steps have counted)
            for _ in range(n_full):
                self._replay()
        if tail:                                             # the short last batch (utils.py:462-463), issued eagerly
            eps, g = host_feed(tail) if host_noise else (None, None)
            inv_B = 1.0 / tail
            eng.train_step(rows, perm, tail, eps, g, first=n_full * b, grad_sync=sync, grad_scale=ex.grad_scale, inv_B=inv_B)
        import time
        t_wall = getattr(self, "_epoch_t0", None)
        torch.cuda.synchronize(sess.device)
        st = eng.read_state()
        loss = float(st.epoch_loss)
        terms = [loss, float(st.epoch_recon), float(st.epoch_klz), float(st.epoch_klc)]
        if world > 1:
            terms = ex.mean_scalars(terms)
            loss = terms[0]
        # what the epoch was made of (the reference prints only the loss; train.py writes these to its metrics log)
        n_rows = n_full * gb + tail
        self.last_epoch = dict(loss=terms[0], recon=terms[1], kl_z=terms[2], kl_c=terms[3], kl_ratio=float(kl_ratio), rows=int(n_rows),
                               steps=int(n_full + (1 if tail else 0)), seconds=(time.perf_counter() - t_wall) if t_wall is not None else None)
        if labels_ptr is not None:
            acc = eng.label_acc()
            if eng.label_err():
                raise RuntimeError("label term: error flag %d (bit 0: a label outside [0, n_classes); bit 1: a row outside the label array)" % eng.label_err())
            # the mean cross-entropy over the labelled rows the epoch saw, how many those were, and how many of them q(c|x) already puts first
            self.last_epoch.update(label_xent=float(acc[0] / acc[1]) if acc[1] else float("nan"), label_rows=int(acc[1]),
                                   label_acc=float(acc[2] / acc[1]) if acc[1] else float("nan"))
        return loss

    # ------------------------------------------------------------------ inference pieces
    def _batches(self, X):
        import torch
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        dev = self._session.device
        b = self._engine.max_batch
        for s in range(0, len(X), b):
            yield s, torch.as_tensor(X[s:s + b]).to(dev)

    def encode(self, X):
        """(mean, log_var, logits) of q(z|x), q(c|x): base_models.py:229-248."""
        eng = self._engine
        out = [[], [], []]
        for _, xb in self._batches(X):
            n = xb.shape[0]
            eng.load_batch(xb, None, 0, n)
            eng.encode(n)
            for k, name in enumerate(("mean", "log_var", "logits")):
                out[k].append(eng.view(name, n).cpu().numpy().copy())
        return tuple(np.concatenate(o, axis=0) for o in out)

    def encode_means_device(self, X):
        """The encoder means of X as one [N][latent_dim] f32 device tensor: every batch's "mean" view is copied on the device,
        nothing returns to the host."""
        import torch
        eng = self._engine
        Z = torch.empty((len(X), self.latent_dim), dtype=torch.float32, device=self._session.device)
        for s, xb in self._batches(X):
            n = xb.shape[0]
            eng.load_batch(xb, None, 0, n)
            eng.encode(n)
            Z[s:s + n].copy_(eng.view("mean", n))
        return Z

    def _fit_prior_on_device(self, X, n_epochs, n_init):
        """gmm="device": the mixture of pretrain_prior (base_models.py:367-390, 614-646) fitted by dmvae_hip.gmm.DiagGMM on the
        device-resident encoder means; deterministic in (Z, seed), so the ranks of a data-parallel run obtain identical tables."""
        from dmvae_hip.gmm import DiagGMM
        gmm_model = DiagGMM(self.n_classes, max_iter=n_epochs, n_init=n_init, weights_init=np.ones(self.n_classes) / self.n_classes,
                            seed=self.seed, seeding=self.gmm_seeding)
        gmm_model.fit(self.encode_means_device(X))
        self._engine.set_parameters({"prior_means": gmm_model.means_,
                                     "prior_log_vars": np.log(gmm_model.covariances_ + 1e-20)})
        return gmm_model

    def _fit_prior_host(self, X, n_epochs, n_init):
        """gmm="host": the same mixture by sklearn on the encoder means (base_models.py:367-390 with n_init = 20, :614-646 with 5)"""
        from sklearn.mixture import GaussianMixture
        gmm_model = GaussianMixture(n_components=self.n_classes, covariance_type="diag", max_iter=n_epochs,
                                    n_init=n_init, weights_init=np.ones(self.n_classes) / self.n_classes)
        gmm_model.fit(self.encode(X)[0])
        self._engine.set_parameters({"prior_means": gmm_model.means_,
                                     "prior_log_vars": np.log(gmm_model.covariances_ + 1e-20)})
        return gmm_model

    def decode(self, Z):
        """reconstructed_X for given Z (what visualization.py:83-87 fetches by feeding model.Z)."""
        import torch
        eng = self._engine
        Z = np.ascontiguousarray(np.asarray(Z, dtype=np.float32))
        out = []
        for s in range(0, len(Z), eng.max_batch):
            zb = torch.as_tensor(Z[s:s + eng.max_batch]).to(self._session.device)
            eng.decode(zb)
            out.append(eng.view("recon", zb.shape[0]).cpu().numpy().copy())
        return np.concatenate(out, axis=0)

    def reconstruct(self, X, epsilon=None):
        """reconstructed_X with the given noise (zeros by default, as
        visualization.py:39-46 feeds): Z = mean + exp(log_var/2) * epsilon."""
        mean, log_var, _ = self.encode(X)
        Z = mean if epsilon is None else mean + np.exp(log_var / 2) * np.asarray(epsilon)
        return self.decode(Z)

    def _eval_order_on_device(self, data, order):
        """the evaluators' upload: the rows `order` of `data` as the int32 permutation _eval_perm on the device, beside the resident rows"""
        import torch
        dev = self._session.device
        t = torch.as_tensor(np.ascontiguousarray(order, dtype=np.int32))
        if self._eval_perm is None or self._eval_perm.numel() != t.numel():      # (a buffer of its own: the captured step holds _perm)
            self._eval_perm = torch.empty(t.numel(), dtype=torch.int32, device=dev)
        self._eval_perm.copy_(t)
        return data.device_rows(dev)

    def _eval_batches(self, data, order):
        """(s, n) of every batch of the rows `order` of `data`, each assembled by load_batch when it is yielded; only enqueues"""
        rows, eng, N = self._eval_order_on_device(data, order), self._engine, len(order)
        for s in range(0, N, eng.max_batch):
            n = min(eng.max_batch, N - s)
            eng.load_batch(rows, self._eval_perm, s, n)
            yield s, n

    def _device_confusion(self, data, order, R, draws=1, eps=None, counter=0):
        """eval="device": the [R, R] confusion matrix [cluster][class] of the rows `order` of `data`, built on the GPU
        (StepEngine.eval_clusters) from the resident rows and classes.  The loop only enqueues -- batch gather, encoder, arg-max
        and count per batch; the matrix and its error flag come back in ONE copy at the end.  eps: VaDE's host noise, flat on
        the device, batch after batch as [draws, n, latent_dim]."""
        eng, dev, D = self._engine, self._session.device, self.latent_dim
        cls = data.device_classes(dev)
        conf = eng.confusion_buffer(R, dev)
        for s, n in self._eval_batches(data, order):
            e = None if eps is None else eps[draws * D * s: draws * D * (s + n)].view(draws, n, D)
            eng.eval_clusters(conf, cls, self._eval_perm, s, n, draws=draws, eps=e, counter=counter)
        return eng.read_confusion(conf)

    def get_accuracy(self, session, data):
        """base_models.py:425-432: logits of every batch -> clustering accuracy.  eval="device": the arg-max and the
        confusion matrix are taken on the GPU from the resident rows (no row, logit or noise crosses the host); the same
        encoder kernels on the same rows, so the matrix -- and the accuracy -- equal the host path's exactly.  Both modes
        reshuffle, so the global NumPy stream and every later epoch are the same."""
        order = data.reshuffle()               # the reference iterates data.get_batches(), which reshuffles
        if self.eval == "device":
            return accuracy_from_confusion(self._device_confusion(data, order, self.n_classes), len(order))
        _, _, logits = self.encode(data.data)   # (the rows in `order`: a binarised data set presents its current draw)
        return get_clustering_accuracy(logits, data._cls[order])

    def get_direct_accuracy(self, session, data):
        """The share of rows whose arg-max cluster IS their class: the trace of the [cluster][class] confusion matrix over N -- no
        matching.  With labels tying cluster c to class c (label_weight) this is the number that matters; get_accuracy stays the
        Hungarian one.  The matrix is the one _device_confusion builds on the GPU, whatever `eval` says.  No reshuffle."""
        order = data.order
        conf = np.asarray(self._device_confusion(data, order, self.n_classes))
        return float(np.trace(conf)) / max(1, len(order))

    def get_log_likelihood(self, session, data, k=50, counter=0):
        """Held-out log-likelihood of `data` in nats per row: the importance-weighted bound (Burda et al., 2016) with k draws of Z per
        row on the marginal mixture prior, computed on the GPU from the resident rows (StepEngine.eval_loglik; k = 1: an ELBO).  The
        same formula for DeepMixtureVAE and VaDE.  Walks the data set in its current order, batch after batch as
        get_accuracy(eval="device") does, WITHOUT reshuffling: nothing is drawn from the NumPy stream.  The noise is the device's
        Philox stream 4 keyed by (seed, counter, draw, position of the row): two calls with one counter return the same bits.
        The loop only enqueues; one float64 pair comes back at the end."""
        eng, N = self._engine, len(data.order)
        acc = eng.loglik_buffer()
        for s, n in self._eval_batches(data, data.order):
            eng.eval_loglik(acc, n, N, s, k, counter=counter)
        return eng.read_loglik(acc)[0]

    _metrics_draws = 1                                     # get_cluster_metrics: the draws eval_clusters averages (VaDE: 10)

    def get_cluster_metrics(self, session, data, silhouette=True, counter=0, return_labels=False):
        """Cluster quality beside the accuracy: dict(acc, nmi, ari, purity, silhouette, n_clusters_used) of `data` (dmvae_hip.metrics).
        acc / nmi / ari / purity come from the confusion matrix [cluster][class] that get_accuracy(eval="device") builds; silhouette
        is the label-free coefficient of the encoder means under the arg-max labels, all pairs on the GPU (csrc/cluster_metrics.hip),
        nan with fewer than 2 (or with n) non-empty clusters.  Walks the data set in its current order WITHOUT reshuffling and draws
        nothing from the NumPy stream; VaDE's responsibilities use the device Philox noise (stream 2, `counter`, 10 draws) whatever
        noise= says.  The loop only enqueues -- gather, encoder and count, the labels, a device copy of the means -- then one
        silhouette call; the matrix, its flag, two doubles and the silhouette's flag come back at the end.  Works with either
        eval= setting.  return_labels: (the dict, the int32 labels of the rows in the evaluated order) instead."""
        return self._cluster_metrics(data, self.n_classes, silhouette, counter, return_labels)

    def _cluster_metrics(self, data, R, silhouette, counter, return_labels):
        import torch
        from dmvae_hip import metrics
        eng, dev = self._engine, self._session.device
        cls = data.device_classes(dev)
        conf = eng.confusion_buffer(R, dev)
        N, D = len(data.order), self.latent_dim
        silhouette = bool(silhouette) and N >= 2
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        Z = torch.empty((N, D), dtype=torch.float32, device=dev) if silhouette else None
        for s, n in self._eval_batches(data, data.order):
            eng.eval_clusters(conf, cls, self._eval_perm, s, n, draws=self._metrics_draws, eps=None, counter=counter)
            eng.eval_labels(labels[s:s + n], n)
            if silhouette:
                Z[s:s + n].copy_(eng.view("mean", n))
        if silhouette:
            _, out, flag = metrics.silhouette_enqueue(Z, labels, self.n_classes)
        d = eng.read_confusion(conf)
        res = metrics.scores_from_confusion(d)
        res["silhouette"] = float("nan")
        res["n_clusters_used"] = int((d.sum(axis=1) > 0).sum())
        if silhouette:
            total, used = out.cpu().tolist()
            if int(flag.item()):
                raise IndexError("cluster metrics on the device: a label outside [0, %d)" % self.n_classes)
            if 2 <= int(used) <= N - 1:
                res["silhouette"] = total / N
        return (res, labels.cpu().numpy()) if return_labels else res

    def get_augmentation_consistency(self, session, data, augment, n_draws=4, seed=0, counter=0):
        """Does a row keep its cluster when it is perturbed?  dict(agree, agree_per_class, acc_clean, acc_aug, n, n_draws) of `data` under
        the random affine maps of `augment` (an AugmentSpec or its string; dmvae_hip.augment, csrc/augment.hip).  One clean pass over the
        resident rows in their current order -- labels through eval_labels, the confusion matrix through eval_clusters -- then, for every
        draw j, the rows warped into ONE scratch buffer under Philox counter counter * n_draws + j and the same batches from it.  agree: the
        share of (row, draw) pairs whose arg-max cluster equals the clean one; agree_per_class: the same per class of the row (nan for a
        class without rows); acc_aug: the accuracy of the warped rows under the CLEAN rows' Hungarian matching, so a drop is a drop and not
        a re-matching.  No reshuffle, nothing drawn from NumPy; VaDE's responsibilities use the device noise of get_cluster_metrics, the
        same for the clean and the warped rows.  The label comparisons are integer ops on the device; everything comes back in one read."""
        import torch
        from scipy.optimize import linear_sum_assignment
        from dmvae_hip.augment import augment as warp, parse_augment
        spec, J = parse_augment(augment), int(n_draws)
        if J < 1:
            raise ValueError("n_draws = %d: at least one draw" % J)
        eng, dev, R = self._engine, self._session.device, self.n_classes
        order = data.order
        N = len(order)
        cls = data.device_classes(dev)
        rows = self._eval_order_on_device(data, order)
        spec.shape_for(rows.shape[1])
        confs = torch.zeros((J + 1, R * R + 1), dtype=torch.int32, device=dev)
        labels = torch.empty((J + 1, N), dtype=torch.int32, device=dev)
        scratch = torch.empty_like(rows)

        def walk(src, j):
            for s in range(0, N, eng.max_batch):
                n = min(eng.max_batch, N - s)
                eng.load_batch(src, self._eval_perm, s, n)
                eng.eval_clusters(confs[j], cls, self._eval_perm, s, n, draws=self._metrics_draws, eps=None, counter=counter)
                eng.eval_labels(labels[j, s:s + n], n)
        walk(rows, 0)
        for j in range(J):
            warp(rows, spec, seed=seed, counter=int(counter) * J + j, out=scratch)
            walk(scratch, j + 1)
        same = (labels[1:] == labels[:1]).sum(dim=0, dtype=torch.int64)                  # [N]: the draws that kept the row's cluster
        c = cls[self._eval_perm.long()].long()
        ok = ((c >= 0) & (c < R)).long()                                                  # (a class outside [0, R) is flagged by eval_clusters)
        c = c.clamp(0, R - 1)
        per = torch.zeros(2 * R, dtype=torch.int64, device=dev)
        per[:R].index_add_(0, c, same * ok)
        per[R:].index_add_(0, c, ok)
        host = torch.cat([confs.reshape(-1).long(), per, same.sum().reshape(1)]).cpu().numpy()       # the one read
        mats = [eng.read_confusion(torch.as_tensor(host[j * (R * R + 1):(j + 1) * (R * R + 1)].astype(np.int32))) for j in range(J + 1)]
        per = host[(J + 1) * (R * R + 1):]
        r, col = linear_sum_assignment(mats[0].max() - mats[0])                           # accuracy_from_confusion's matching, kept for the warped rows
        with np.errstate(invalid="ignore", divide="ignore"):
            per_class = per[:R] / (per[R:2 * R] * float(J))
        return dict(agree=float(per[2 * R]) / (N * J), agree_per_class=[float(x) for x in per_class],
                    acc_clean=float(mats[0][r, col].sum()) / N, acc_aug=float(sum(m[r, col].sum() for m in mats[1:])) / (N * J), n=int(N), n_draws=J)

    def get_posterior_diagnostics(self, session, data, counter=0, max_points=None, au_threshold=0.01, eps=None, return_points=False):
        """What the KL term bought: dict(mi, marginal_kl, rate, mi_cap, active_units, var_of_mean, mean_of_var, n_points, n_rows) of
        `data` (dmvae_hip.density, csrc/mixture_density.hip).  With z_i ~ q(z|x_i) one sample per point, a_i = log q(z_i|x_i),
        m_i = log q(z_i) under the aggregate posterior 1/N sum_n q(z|x_n) over ALL n_rows rows (the row itself included) and p_i = log p(z_i)
        under the marginal mixture prior: mi = mean(a - m), the estimate of I(x;z) of He et al. 2019, at most mi_cap = log n_rows;
        marginal_kl = mean(m - p), the mismatch KL(q(z) || p(z)); rate = mean(a - p), their sum (Hoffman & Johnson 2016).
        var_of_mean[d] / mean_of_var[d]: the population variance of the encoder means / the mean encoder variance of dimension d;
        active_units = #{d: var_of_mean[d] > au_threshold} (Burda et al. 2016).  max_points = M < n_rows scores the rows floor(i n_rows / M)
        only (still against all rows).  Walks the data set in its current order WITHOUT reshuffling, draws nothing from NumPy and writes
        no parameter, moment or step state: the noise is eps ([n_points][latent_dim], NumPy or device) or the device's Philox stream 6
        keyed by (seed, counter).  The loop only enqueues -- gather, encoder, device copies of the mean and log_var views -- then the
        sample, two all-pairs log-density calls, the column statistics and three float64 sums; one small copy comes back at the end.
        return_points: (the dict, z [n_points][latent_dim], a [n_points]) with the device tensors of the sample instead."""
        import torch
        from dmvae_hip import density
        eng, dev = self._engine, self._session.device
        N, D = len(data.order), self.latent_dim
        mean = torch.empty((N, D), dtype=torch.float32, device=dev)
        log_var = torch.empty((N, D), dtype=torch.float32, device=dev)
        for s, n in self._eval_batches(data, data.order):
            eng.encode(n)
            mean[s:s + n].copy_(eng.view("mean", n))
            log_var[s:s + n].copy_(eng.view("log_var", n))
        if eps is not None and not isinstance(eps, torch.Tensor):
            eps = torch.as_tensor(np.ascontiguousarray(np.asarray(eps, dtype=np.float32))).to(dev)
        enq = density.posterior_diagnostics_enqueue(mean, log_var, eng.param_view("prior_means"), eng.param_view("prior_log_vars"), seed=self.seed,
                                                    counter=counter, max_points=max_points, eps=eps)
        res = density.diagnostics_from(enq, au_threshold)
        return (res, enq["z"], enq["a"]) if return_points else res

    def _eval_means_device(self, data):
        """the encoder means of `data` in its current order as one [N][latent_dim] f32 device tensor (_eval_perm then holds that order);
        only enqueues: gather, encoder and a device copy of the "mean" view per batch"""
        import torch
        eng = self._engine
        Z = torch.empty((len(data.order), self.latent_dim), dtype=torch.float32, device=self._session.device)
        for s, n in self._eval_batches(data, data.order):
            eng.encode(n)
            Z[s:s + n].copy_(eng.view("mean", n))
        return Z

    def get_knn_accuracy(self, session, train_data, test_data, k=10, return_confusion=False):
        """Are rows of one class close in latent space, whatever the clusters did with them?  The accuracy of sklearn's uniform-weight
        k-nearest-neighbour classifier (Euclidean, brute force) fitted on the encoder means of `train_data` and asked about those of
        `test_data`: all pairs on the GPU (dmvae_hip.knn, csrc/knn.hip), an exact distance tie going to the earlier train row in the
        evaluated order and a tied vote to the smallest class.  Walks both data sets in their current order WITHOUT reshuffling and
        draws nothing from the NumPy stream.  The loop only enqueues -- gather, encoder, a device copy of the means -- then the
        neighbours, the vote, the arg-max and the count against the resident classes; the matrix and its flag come back in ONE copy.
        return_confusion: (accuracy, the int64 matrix [predicted class][class]) instead."""
        from dmvae_hip import knn
        eng, dev = self._engine, self._session.device
        n_train, n_test = len(train_data.order), len(test_data.order)
        if not 1 <= int(k) <= min(knn.MAX_K, n_train):
            raise ValueError("k = %d: 1 <= k <= min(%d, the %d train rows)" % (k, knn.MAX_K, n_train))
        R = int(max(np.max(train_data._cls), np.max(test_data._cls))) + 1
        Zx = self._eval_means_device(train_data)
        cls_x = train_data.device_classes(dev)[self._eval_perm.long()]       # the classes of the database rows, in the evaluated order
        Zq = self._eval_means_device(test_data)
        conf = eng.confusion_buffer(R, dev)
        idx, _ = knn.knn_enqueue(Zq, Zx, int(k))
        counts, _ = knn.vote_enqueue(idx, cls_x, R, flag=conf[R * R:])
        eng.confusion_add(conf, counts, test_data.device_classes(dev), self._eval_perm, 0, n_test)
        d = eng.read_confusion(conf)
        acc = float(np.trace(d)) / n_test
        return (acc, d) if return_confusion else acc

    def get_linear_probe_accuracy(self, session, train_data, test_data, C=1.0, tol=1e-4, max_iter=200, standardize=True, return_confusion=False):
        """Are the classes linearly separable in latent space?  The accuracy on `test_data` of a multinomial logistic regression (the
        "linear probe": sklearn's LogisticRegression objective, inverse penalty C) fitted on the encoder means of `train_data`: loss and
        gradient of every L-BFGS evaluation in one pass over the rows on the GPU (dmvae_hip.probe, csrc/probe.hip).  Where kNN is local
        and depends on the metric, the probe is global and indifferent to an invertible linear map of z.  Walks both data sets in their
        current order WITHOUT reshuffling and draws nothing from the NumPy stream.  standardize: the train means' column mean and
        1 / std reach the kernels as shift and scale.  The test means' scores go to the arg-max count against the resident classes (a
        tie to the smaller class); the matrix and its flag come back in ONE copy.  The fitted probe stays in last_linear_probe_.
        return_confusion: (accuracy, the int64 matrix [predicted class][class]) instead."""
        from dmvae_hip import probe
        eng, dev = self._engine, self._session.device
        n_test = len(test_data.order)
        R = int(max(np.max(train_data._cls), np.max(test_data._cls))) + 1
        Zx = self._eval_means_device(train_data)
        cls_x = train_data.device_classes(dev)[self._eval_perm.long()]       # the classes of the fit rows, in the evaluated order
        Zq = self._eval_means_device(test_data)
        clf = probe.LogisticRegression(C=C, tol=tol, max_iter=max_iter, standardize=standardize, n_classes=max(R, 2)).fit(Zx, cls_x)
        self.last_linear_probe_ = clf
        conf = eng.confusion_buffer(max(R, 2), dev)
        eng.confusion_add(conf, clf.decision_function(Zq), test_data.device_classes(dev), self._eval_perm, 0, n_test)
        d = eng.read_confusion(conf)[:R, :R]
        acc = float(np.trace(d)) / n_test
        return (acc, d) if return_confusion else acc

    def get_few_label_accuracy(self, session, train_data, test_data, n_labeled=100, seed=0, k=7, alpha=0.8, weights="connectivity", labeled=None):
        """Given this latent space and only n_labeled labels, how many test rows end up with the right class -- and how much of that comes
        from the unlabelled rows?  Label spreading (Zhou et al. 2004; dmvae_hip.spread, csrc/label_spread.hip) over ONE symmetric k-nearest-
        neighbour graph of the encoder means of the train rows followed by the test rows, both in the data sets' own unpermuted numbering.
        Labels: the rows choose_labeled(train classes, n_labeled, n_classes, seed) of the train data and nobody else; labeled: these row
        indices instead (Dataset.labeled of a semi-supervised run).  Returns dict(accuracy: over the test rows; accuracy_unlabeled_train:
        over the train rows without a label; n_unreached: rows of the graph no label reaches -- they count as wrong; n_iter, change: of
        the iteration; per_class: the test accuracy per class (nan for a class without test rows); knn1 and probe: on the SAME labels and
        nothing else, the test accuracy of the 1-nearest-neighbour classifier and of the linear probe fitted on the labelled means alone
        -- accuracy minus these is what the unlabelled geometry adds; n_labeled).  No reshuffle, nothing drawn from the NumPy stream, no
        parameter or step state written.  ValueError when a class lacks its quota of rows or k does not fit the rows."""
        import torch
        from dmvae_hip import knn, probe, spread
        from includes.utils import choose_labeled
        n_train, n_test = len(train_data.order), len(test_data.order)
        cls_x, cls_q = np.asarray(train_data._cls).astype(np.int64), np.asarray(test_data._cls).astype(np.int64)
        R = int(max(np.max(cls_x), np.max(cls_q))) + 1
        if labeled is None:
            labeled = choose_labeled(cls_x, n_labeled, R, seed)
        labeled = np.unique(np.asarray(labeled, dtype=np.int64))
        if len(labeled) < 1 or labeled[0] < 0 or labeled[-1] >= n_train:
            raise ValueError("get_few_label_accuracy: the labelled rows must be train rows in [0, %d), one at least" % n_train)
        Z = torch.empty((n_train + n_test, self.latent_dim), dtype=torch.float32, device=self._session.device)
        for data, at in ((train_data, 0), (test_data, n_train)):
            for s, n in self._eval_batches(data, np.arange(len(data.order))):
                self._engine.encode(n)
                Z[at + s:at + s + n].copy_(self._engine.view("mean", n))
        y = np.full(n_train + n_test, -1, dtype=np.int64)
        y[labeled] = cls_x[labeled]
        ls = spread.LabelSpreading(n_neighbors=k, alpha=alpha, weights=weights).fit(Z, y)
        self.last_label_spreading_ = ls
        truth = np.concatenate([cls_x, cls_q])
        ok = ls.transduction_ == truth
        free = np.ones(n_train, dtype=bool)
        free[labeled] = False
        per_class = [float(np.mean(ok[n_train:][cls_q == c])) if np.any(cls_q == c) else float("nan") for c in range(R)]
        Zl, Zq, yl = Z[torch.as_tensor(labeled, device=Z.device)], Z[n_train:], cls_x[labeled]
        knn1 = knn.KNeighborsClassifier(n_neighbors=1).fit(Zl, yl).score(Zq, cls_q)
        if len(np.unique(yl)) >= 2:
            lin = float(np.mean(probe.LogisticRegression(C=1.0, tol=1e-4, max_iter=200, standardize=True).fit(Zl, yl).predict(Zq) == cls_q))
        else:
            lin = float(np.mean(cls_q == yl[0]))                     # one class among the labels: the probe has nothing to separate
        return dict(accuracy=float(np.mean(ok[n_train:])), accuracy_unlabeled_train=float(np.mean(ok[:n_train][free])) if free.any() else float("nan"),
                    n_unreached=ls.n_unreached_, n_iter=ls.n_iter_, change=ls.change_, per_class=per_class, knn1=knn1, probe=lin,
                    n_labeled=int(len(labeled)))

    def get_latent_map(self, session, data, perplexity=30.0, n_iter=1000, method="auto", trust_neighbors=5, counter=0):
        """The map of the latent space: the t-SNE of the encoder means of ALL rows of `data` on the GPU (dmvae_hip.tsne.TSNE), with what a
        plot colours it by.  method: "exact" (the dense P, up to 32768 rows), "knn" (P over the int(3 perplexity + 1) nearest rows, the
        repulsion exact over all pairs, up to 2^20 rows) or "auto": exact up to 32768 rows, knn above.  Returns dict(embedding [N][2] f32,
        classes [N], clusters [N] -- the arg-max of the scores as eval="device" takes it -- all three in the data set's current order, kl,
        trustworthiness (sklearn.manifold.trustworthiness of the embedding against the means with trust_neighbors neighbours,
        dmvae_hip.knn), method (what ran), n_neighbors (of the knn form, else None), seconds).  Walks the data set in its current order
        WITHOUT reshuffling and draws nothing from the NumPy stream: the start is the device's Philox stream 5 keyed by the model's seed,
        VaDE's responsibilities use Philox stream 2 keyed by `counter`.  Two calls return the same bits."""
        return self._latent_map(data, self.n_classes, perplexity, n_iter, method, trust_neighbors, counter)

    def _latent_map(self, data, R, perplexity, n_iter, method, trust_neighbors, counter):
        import time
        import torch
        from dmvae_hip import tsne
        if method not in ("auto", "exact", "knn"):
            raise ValueError("method must be 'auto', 'exact' or 'knn'")
        dev, N = self._session.device, len(data.order)
        how = method if method != "auto" else ("exact" if N <= tsne.EXACT_MAX_N else "knn")
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        R = max(int(R), int(np.max(data._cls)) + 1)          # (the map does not need the classes to fit the clusters' matrix)
        _, clusters = self._cluster_metrics(data, R, False, counter, True)
        Z = self._eval_means_device(data)
        classes = np.asarray(data._cls)[np.asarray(data.order)]
        t = tsne.TSNE(perplexity=perplexity, n_iter=n_iter, random_state=self.seed, method=how).fit(Z)
        trust = t.trustworthiness(Z, trust_neighbors)
        return dict(embedding=t.embedding_, classes=classes, clusters=clusters, kl=t.kl_divergence_, trustworthiness=trust, method=how,
                    n_neighbors=t.n_neighbors_ if how == "knn" else None, seconds=time.perf_counter() - t0)

    def get_cluster_exemplars(self, session, data, n=10):
        """The real rows that live in each cluster: an int array [n_classes][n] whose entry [c] holds the rows of `data`, in the data
        set's own unpermuted numbering, whose encoder means are nearest prior mean c, nearest first (a tie to the row that comes
        earlier in the current order).  No reshuffle; dmvae_hip.knn on the device, one copy back."""
        from dmvae_hip import knn
        Z = self._eval_means_device(data)
        idx, _ = knn.kneighbors(self._engine.param_view("prior_means"), Z, int(n))
        return self._eval_perm.long()[idx.long()].cpu().numpy().astype(np.int64)

    def sample_prior_device(self, n, counter=0):
        """(rows f32 [n][input_dim], latents f32 [n][latent_dim], components int32 [n]) on the device: decoded draws from the mixture
        prior.  Row j comes from component c = j mod n_classes: z_j = mu_c + exp(lv_c / 2) eps_j with eps_j[d] = element j latent_dim + d
        of the Philox stream (the model's seed, step = counter, stream id 7) of dmvae_philox_normal, and the row is the decoder's MEAN
        image of z_j (the "recon" view), not a Bernoulli draw from it.  Only enqueues: the draw, then a decode and a device copy of
        "recon" per batch."""
        import torch
        from dmvae_hip import prdc
        eng, dev, D, K, n = self._engine, self._session.device, self.latent_dim, self.n_classes, int(n)
        comp = torch.arange(n, device=dev) % K
        eps = prdc.philox_normal(n * D, self.seed, step=counter, device=dev).view(n, D)
        Z = (eng.param_view("prior_means").float()[comp] + torch.exp(eng.param_view("prior_log_vars").float()[comp] / 2) * eps).contiguous()
        X = torch.empty((n, self.input_dim), dtype=torch.float32, device=dev)
        for s in range(0, n, eng.max_batch):
            b = min(eng.max_batch, n - s)
            eng.decode(Z[s:s + b])
            X[s:s + b].copy_(eng.view("recon", b))               # (casts a bf16 plan's view to f32)
        return X, Z, comp.to(torch.int32)

    def _real_and_generated_features(self, data, M, space, counter):
        """what get_sample_quality and get_sample_distance compare: (R f32 [N][D] of the rows of `data` in their current order, F f32 [M][D]
        of the M rows of sample_prior_device(M, counter), the component of every generated row, the class of every real row -- or None -- and
        the number of classes).  space="latent": encoder means on both sides; "input": the rows themselves.  Only enqueues."""
        import torch
        eng, dev = self._engine, self._session.device
        X, _, comp = self.sample_prior_device(M, counter)
        if space == "latent":
            F = torch.empty((M, self.latent_dim), dtype=torch.float32, device=dev)
            for s in range(0, M, eng.max_batch):
                n = min(eng.max_batch, M - s)
                eng.load_batch(X, None, s, n)
                eng.encode(n)
                F[s:s + n].copy_(eng.view("mean", n))
            R = self._eval_means_device(data)
        else:
            rows = self._eval_order_on_device(data, data.order)
            R, F = rows[self._eval_perm.long()], X
        cls = getattr(data, "_cls", None)
        real_groups = n_groups = None
        if cls is not None and np.issubdtype(np.asarray(cls).dtype, np.integer) and len(cls) == len(data.order):
            real_groups, n_groups = data.device_classes(dev)[self._eval_perm.long()], int(np.max(cls)) + 1
        return R, F, comp, real_groups, n_groups

    def get_sample_quality(self, session, data, k=5, n_samples=None, space="latent", counter=0):
        """Are the decoded draws from the mixture prior p(z) = 1/K sum_c N(mu_c, diag exp(lv_c)) realistic, and do they cover the data?
        Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of M generated rows
        against the N rows of `data`, all pairs on the GPU (dmvae_hip.prdc, csrc/prdc.hip), k-th-neighbour balls closed, squared radii
        from dmvae_knn.  Returns dict(precision, recall, density, coverage, k, n_real, n_samples, space,
        precision_per_cluster [K], density_per_cluster [K]) -- which component generates junk -- and, when `data` holds classes,
        coverage_per_class and recall_per_class -- which classes the prior misses (nan for a class without rows).
        Generated rows: M = n_samples, by default N rounded down to a multiple of K; row j comes from component j mod K (the uniform
        prior of the KL_C term), z = mu_c + exp(lv_c / 2) eps with eps from the device's Philox stream 7 keyed by (seed, counter),
        decoded in batches.  A generated row is the decoder's MEAN image (the "recon" view), not a Bernoulli draw from it.
        space="latent" (default): features are encoder means -- of the real rows, and of the generated rows encoded again;
        space="input": the rows themselves, D = input_dim.  Walks `data` in its current order WITHOUT reshuffling and draws nothing
        from the NumPy stream; writes no parameter, moment or step state.  The loop only enqueues; one copy comes back at the end.
        ValueError unless 1 <= k <= min(256, N - 1, M - 1) and space is one of the two."""
        from dmvae_hip import prdc
        if space not in ("latent", "input"):
            raise ValueError("space = %r: 'latent' or 'input'" % (space,))
        K, N = self.n_classes, len(data.order)
        M = (N // K) * K if n_samples is None else int(n_samples)
        if not 1 <= int(k) <= min(256, N - 1, M - 1):
            raise ValueError("k = %d: 1 <= k <= min(256, the %d real rows - 1, the %d generated rows - 1)" % (k, N, M))
        R, F, comp, real_groups, n_groups = self._real_and_generated_features(data, M, space, counter)
        flat, layout = prdc.prdc_enqueue(R, F, int(k), real_groups, comp, n_groups, K)
        res = prdc.prdc_from(flat, layout, N, M, int(k))
        res["precision_per_cluster"], res["density_per_cluster"] = np.array(res.pop("precision_per_group")), np.array(res.pop("density_per_group"))
        if real_groups is not None:
            res["coverage_per_class"], res["recall_per_class"] = np.array(res.pop("coverage_per_group")), np.array(res.pop("recall_per_group"))
        res.update(n_real=N, n_samples=M, space=space)
        return res

    def get_sample_distance(self, session, data, eps_rel=0.05, n_samples=None, space="latent", counter=0, tol=1e-4, max_iter=500):
        """How far is the distribution of the decoded draws from the mixture prior from the distribution of the data?  The Sinkhorn
        divergence S_eps (Feydy et al. 2019; debiased entropic optimal transport, cost = squared Euclidean distance, no 1/2: S_eps -> W_2^2
        as eps -> 0) between M generated rows and the N rows of `data`, both uniformly weighted, on the GPU (dmvae_hip.sinkhorn,
        csrc/sinkhorn.hip): 0 when the two coincide, in squared-distance units of the chosen space, no assumption on the clouds' shape.
        eps = eps_rel x the mean squared distance over all pairs.  Returns dict(divergence, ot, eps, n_iter, err, n_real, n_samples, space,
        per_cluster [K], mean_per_cluster [K]) -- the share of the divergence carried by the rows of each prior component and that share per
        unit of mass: which component generates far from the data -- and, when `data` holds classes, per_class and mean_per_class -- which
        classes are far from anything the prior generates (a class without rows: 0 and nan).  per_cluster and per_class together add up to
        the divergence; a single entry may be negative.  n_iter and err: iterations (annealing included) and final marginal residual of the
        three transport problems (data against samples, data against itself, samples against themselves).
        The two row sets are those of get_sample_quality at the same arguments: M = n_samples, by default N rounded down to a multiple of K,
        row j from component j mod K, z = mu_c + exp(lv_c / 2) eps with eps from the device's Philox stream 7 keyed by (seed, counter), the
        decoder's MEAN image; space="latent" (default): encoder means of both sets, space="input": the rows themselves.  Walks `data` in its
        current order WITHOUT reshuffling and draws nothing from the NumPy stream; writes no parameter, moment or step state.
        ValueError unless space is one of the two, M >= 1, eps_rel > 0, tol >= 0 and max_iter >= 1."""
        from dmvae_hip import sinkhorn
        if space not in ("latent", "input"):
            raise ValueError("space = %r: 'latent' or 'input'" % (space,))
        K, N = self.n_classes, len(data.order)
        M = (N // K) * K if n_samples is None else int(n_samples)
        if M < 1 or not float(eps_rel) > 0 or not tol >= 0 or int(max_iter) < 1:
            raise ValueError("n_samples = %d, eps_rel = %r, tol = %r, max_iter = %r: M >= 1, eps_rel > 0, tol >= 0, max_iter >= 1" % (M, eps_rel, tol, max_iter))
        R, F, comp, real_groups, n_groups = self._real_and_generated_features(data, M, space, counter)
        sd = sinkhorn.sinkhorn_divergence(R, F, eps_rel=eps_rel, tol=tol, max_iter=max_iter, real_groups=real_groups, fake_groups=comp,
                                          n_real_groups=n_groups, n_fake_groups=K)
        res = dict(divergence=sd["divergence"], ot=sd["ot"], eps=sd["eps"], n_iter=sd["n_iter"], err=sd["err"], n_real=N, n_samples=M, space=space,
                   per_cluster=np.array(sd["per_fake_group"]), mean_per_cluster=np.array(sd["mean_per_fake_group"]))
        if real_groups is not None:
            res.update(per_class=np.array(sd["per_real_group"]), mean_per_class=np.array(sd["mean_per_real_group"]))
        return res

    def get_reconstruction_quality(self, session, data, image_shape=None, n_worst=10, window=None, data_range=1.0, return_images=False):
        """How good are the reconstructions, and for which rows are they bad?  The structural similarity (Wang et al. 2004) of every row
        of `data` with its reconstruction -- the decoder's mean image of the encoder's mean, epsilon = 0: the images reconstruct(X)
        returns -- on the GPU (dmvae_hip.ssim, csrc/ssim.hip: valid windows, centred moments), beside the mean squared error.  Returns
        dict(ssim, mse, psnr, n, image_shape, worst, worst_ssim) and, when `data` holds classes, ssim_per_class and mse_per_class (nan for a
        class without rows).  ssim and mse are the means over the rows, psnr = 10 log10(data_range^2 / mse) of that mean mse (inf at 0);
        worst: the n_worst rows of lowest SSIM in the data set's own numbering, lowest first, a tie going to the row evaluated earlier
        (a stable sort); worst_ssim their values.  image_shape: (H, W) or (planes, H, W); None means (sqrt(input_dim), sqrt(input_dim)),
        a ValueError when input_dim is no perfect square.  window: the 1-D weights of the separable window (default: Gaussian, 11 taps,
        sigma 1.5).  Walks `data` in its current order WITHOUT reshuffling and draws nothing from the NumPy stream; writes no parameter,
        moment or step state.  Per batch: gather, encode, decode the "mean" view, an f32 copy of "recon", one dmvae_ssim_rows launch that
        reads the resident rows through the evaluated order.  The loop only enqueues; one f32 vector [ssim | sse] comes back at the end
        and the group means are taken from it on the host in float64 (np.bincount: a device index_add_ would be a float atomic).
        return_images: (the dict, the reconstructions f32 [n][input_dim] on the device, in the evaluated order) instead."""
        import torch
        from dmvae_hip import ssim as S
        shape = S._plane_shape(S.default_image_shape(self.input_dim) if image_shape is None else image_shape, self.input_dim)
        S._window(window, shape[1], shape[2])
        eng, dev, N = self._engine, self._session.device, len(data.order)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        parts_s, parts_e, images = [], [], []
        rows = data.device_rows(dev)
        for s, n in self._eval_batches(data, data.order):
            eng.encode(n)
            Z = torch.empty((n, self.latent_dim), dtype=torch.float32, device=dev)
            Z.copy_(eng.view("mean", n))
            eng.decode(Z)
            Y = torch.empty((n, self.input_dim), dtype=torch.float32, device=dev)
            Y.copy_(eng.view("recon", n))                        # (casts a bf16 plan's view to f32)
            sv, ev = S.ssim_enqueue(rows, Y, shape, ix=self._eval_perm[s:s + n], window=window, data_range=data_range, flag=flag)
            parts_s.append(sv)
            parts_e.append(ev)
            if return_images:
                images.append(Y)
        host = torch.cat(parts_s + parts_e + [flag.view(torch.float32)]).cpu().numpy()
        if int(host[2 * N:].view(np.int32)[0]):
            raise IndexError("reconstruction quality on the device: a row index out of range")
        sv, mse_rows, _ = S.quality_from(host[:N], host[N:2 * N], self.input_dim, data_range)
        mse = float(mse_rows.mean())
        idx = np.argsort(sv, kind="stable")[:max(0, int(n_worst))]
        res = dict(ssim=float(sv.mean()), mse=mse, psnr=float("inf") if mse == 0.0 else float(10.0 * np.log10(float(data_range) ** 2 / mse)), n=N,
                   image_shape=shape if image_shape is not None and len(tuple(image_shape)) == 3 else shape[1:],
                   worst=np.asarray(data.order)[idx].astype(np.int64), worst_ssim=sv[idx])
        cls = getattr(data, "_cls", None)
        if cls is not None and np.issubdtype(np.asarray(cls).dtype, np.integer) and len(cls) == len(data.order):
            g, G = np.asarray(cls)[data.order], int(np.max(cls)) + 1
            count = np.bincount(g, minlength=G)
            with np.errstate(invalid="ignore", divide="ignore"):
                res["ssim_per_class"] = np.bincount(g, weights=sv, minlength=G) / count
                res["mse_per_class"] = np.bincount(g, weights=mse_rows, minlength=G) / count
        return (res, torch.cat(images)) if return_images else res

    def get_sample_diversity(self, session, n_per_cluster=32, image_shape=None, counter=0, collapsed_above=0.9, window=None, data_range=1.0):
        """Has a mixture component collapsed onto one image, or do two components generate the same thing?  The mean pairwise SSIM among
        decoded draws from the prior (Odena et al. 2017), per component, on the GPU (dmvae_hip.ssim.pairwise_enqueue).  The draws are
        sample_prior_device(n_per_cluster K, counter): the samples get_sample_quality judges at the same counter, row j from component
        j mod K.  Returns dict(ssim_within [K], ssim_between, ssim_between_per_cluster [K], collapsed, n_per_cluster, image_shape):
        ssim_within[c] = the mean SSIM over all n_per_cluster (n_per_cluster - 1) / 2 pairs of component c's draws (1 = one image);
        ssim_between = the mean over the pairs (draw t of c, draw t of c') for c < c' and all t, ssim_between_per_cluster[c] the mean over
        those of them that involve c (nan for K = 1); collapsed = the components whose within-value exceeds collapsed_above -- 0.9 is a
        convention, not a theorem: distinct MNIST digits of one class lie near 0.2 - 0.5.  Draws nothing from the NumPy stream and writes
        no parameter, moment or step state.  Only enqueues; one f32 vector comes back at the end, the means are float64 on the host.
        ValueError unless n_per_cluster >= 2."""
        import torch
        from dmvae_hip import ssim as S
        shape = S._plane_shape(S.default_image_shape(self.input_dim) if image_shape is None else image_shape, self.input_dim)
        S._window(window, shape[1], shape[2])
        K, m, dev = self.n_classes, int(n_per_cluster), self._session.device
        if m < 2:
            raise ValueError("n_per_cluster = %d: a component needs two draws for a pair" % m)
        X, _, _ = self.sample_prior_device(m * K, counter)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        comp = np.arange(m * K) % K
        sw, _, _, _, _ = S.pairwise_enqueue(X, comp, K, shape, window=window, data_range=data_range, flag=flag)
        parts = [sw]
        if K > 1:
            ca, cb = np.triu_indices(K, 1)                       # the pairs c < c', for every t: rows t K + c and t K + c'
            base = (np.arange(m) * K)[:, None]
            sb, _ = S.ssim_enqueue(X, X, shape, ix=(base + ca[None, :]).reshape(-1), iy=(base + cb[None, :]).reshape(-1), window=window,
                                   data_range=data_range, flag=flag)
            parts.append(sb)
        host = torch.cat(parts + [flag.view(torch.float32)]).cpu().numpy()
        if int(host[-1:].view(np.int32)[0]):
            raise IndexError("sample diversity on the device: a row index out of range")
        P = m * (m - 1) // 2
        within = host[:K * P].astype(np.float64).reshape(K, P).mean(axis=1)
        between, per = float("nan"), np.full(K, np.nan)
        if K > 1:
            vb = host[K * P:-1].astype(np.float64).reshape(m, len(ca))
            between = float(vb.mean())
            per = np.array([vb[:, (ca == c) | (cb == c)].mean() for c in range(K)])
        return dict(ssim_within=within, ssim_between=between, ssim_between_per_cluster=per,
                    collapsed=[int(c) for c in np.nonzero(within > float(collapsed_above))[0]], n_per_cluster=m,
                    image_shape=shape if image_shape is not None and len(tuple(image_shape)) == 3 else shape[1:])

    # ------------------------------------------------------------------ pretraining (base_models.py:304-423)
    # the variables tf.get_collection(TRAINABLE_VARIABLES, scope=name + "/encoder_network/c") returns (:313-315)
    PRIOR_VAR_LIST = ("W_ch", "b_ch", "W_logits", "b_logits")

    def define_pretrain_step(self, vae_lr, prior_lr):
        """base_models.py:304-320: two more Adam optimizers, each with its own slots --
        vae_train_step = Adam(vae_lr).minimize(recon_loss) over every variable the
        reconstruction depends on, prior_train_step = Adam(prior_lr).minimize(latent_loss,
        var_list = the c-head)."""
        self.define_train_loss()
        self.vae_loss = "recon"
        self._vae_lr, self._prior_lr = float(vae_lr), float(prior_lr)
        self.vae_train_step = "adam_tf(recon_loss)"
        self.prior_train_step = "adam_tf(latent_loss, var_list=encoder_network/c)"

    def _ckpt(self, stage):
        return os.path.join(self.path, stage, "parameters.npz") if self.path else None

    def _restore(self, stage):
        """the reference wraps its restore in try / except and carries on (base_models.py:324-329, :354-359)"""
        path = self._ckpt(stage)
        if not (path and os.path.exists(path)):
            return False
        try:
            with np.load(path, allow_pickle=False) as f:
                self.load_state_dict({k: f[k] for k in f.files})
            return True
        except (OSError, ValueError, KeyError, RuntimeError, EOFError, zipfile.BadZipFile) as e:
            print("Could not read %s: %s" % (path, e))
            return False

    def _save(self, stage):
        """rank 0 writes (to a temporary file, then an atomic rename); the other ranks wait at a barrier
        so that none of them reads a half-written archive"""
        path = self._ckpt(stage)
        if not path:
            return
        sess = self._session
        if sess is not None and sess.world_size > 1:      # sharded bf16 steps leave a rank's fp32 weights current on its own slice only
            from dmvae_hip import make_exchange
            self._engine.sync_master(make_exchange(4 * self._engine.param.numel()))      # collective: every rank is here
        if sess is None or sess.rank == 0:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tmp = path + ".tmp.npz"
            np.savez(tmp, **self.state_dict())
            os.replace(tmp, path)
        if sess is not None and sess.world_size > 1:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                dist.barrier()

    def _pretrain_epoch(self, sess, data, stage):
        """one epoch of a pretraining stage: epsilon = 0 (so Z = mean), the stage's loss and
        variable list; returns sum(batch_loss) / epoch_len like the reference's loops (:331-350, :395-414)."""
        import torch
        from dmvae_hip import make_exchange
        eng = self._engine
        world = sess.world_size
        b = data.batch_size // world
        if data.batch_size % world or b != eng.max_batch:
            raise ValueError("batch_size %d does not match the model (%d per rank x %d ranks)" % (data.batch_size, eng.max_batch, world))
        rows = data.train_rows(sess.device)                    # (device_rows itself unless the data set augments: DESIGN.md section 30)
        self._bind_labels(sess, data, train=False)             # (an attached plan pretrains at w = 0)
        perm, n_full, tail, weight = self._epoch_perm(data, sess)
        import time
        torch.cuda.synchronize(sess.device)
        self._epoch_t0 = time.perf_counter()                   # (behind the row upload and the epoch's permutation: the steps themselves)
        ex = make_exchange(4 * eng.param.numel())
        sync = ex if ex.enabled else None
        # recon-only objective = the full loss at kl_ratio 0: every KL gradient carries the factor r
        eng.reset_epoch(n_full + (1 if tail else 0), kl_ratio=0.0 if stage == "vae" else 1.0, epoch_weight=weight)
        zeros = {}

        def noise(n):
            if n not in zeros:
                zeros[n] = (torch.zeros((n, self.latent_dim), dtype=torch.float32, device=sess.device),
                            torch.zeros((n, self.n_classes), dtype=torch.float32, device=sess.device) if self.gumbel else None)
            return zeros[n]
        frozen = [k for k in eng.parameter_names() if k not in self.PRIOR_VAR_LIST]
        for i in range(n_full + (1 if tail else 0)):
            n = b if i < n_full else tail
            inv_B = (world / float(data.batch_size)) if i < n_full else 1.0 / n
            eps, g = noise(n)
            if stage == "vae":
                eng.train_step(rows, perm, n, eps, g, first=i * b, grad_sync=sync, grad_scale=ex.grad_scale, inv_B=inv_B)
            else:
                eng.load_batch(rows, perm, i * b, n)
                eng.forward_backward(n, eps, g, inv_B)
                if sync is not None:
                    sync(eng.grad)
                for k in frozen:                      # minimize(..., var_list=c-head): nothing else moves
                    eng.grad_view(k).zero_()
                eng.update(ex.grad_scale)
        torch.cuda.synchronize(sess.device)
        st = eng.read_state()
        loss = float(st.epoch_recon) if stage == "vae" else float(st.epoch_klz) + float(st.epoch_klc)
        if world > 1:
            loss = ex.mean_scalars([loss])[0]
        self._replay = None        # the step graph was captured for the main optimizer's state; recapture after pretraining
        return loss

    def _sync_master(self, sess):
        """COLLECTIVE under data parallelism (every rank calls it at the same point): bring the fp32 master weights up to date on
        every rank after sharded bf16 steps, before anything reads or rewrites the whole fp32 arena (StepEngine.sync_master)."""
        if sess is not None and sess.world_size > 1:
            from dmvae_hip import make_exchange
            self._engine.sync_master(make_exchange(4 * self._engine.param.numel()))

    def pretrain_vae(self, session, data, n_epochs):
        """base_models.py:322-350."""
        sess = session or self._session
        if not self._restore("vae"):
            print("Could not load trained ae parameters")
        self._engine.reset_optimizer(self._vae_lr)
        min_loss = float("inf")
        for _ in range(n_epochs):
            loss = self._pretrain_epoch(sess, data, "vae")
            if loss <= min_loss:
                min_loss = loss
                self._save("vae")
        self._sync_master(sess)       # the next stage sets parameters / runs the replicated Adam over the whole fp32 arena
        return min_loss

    def pretrain_prior(self, session, data, n_epochs):
        """base_models.py:352-414: prior tables from a diagonal GMM on the encoder means, then
        Adam on the latent loss over the c-head only."""
        sess = session or self._session
        if not self._restore("prior"):
            print("Could not load trained prior parameters")
            if n_epochs > 0 and self.gmm == "device":
                self._fit_prior_on_device(data.data, n_epochs, n_init=20)
                self._save("prior")
            elif n_epochs > 0:
                self._fit_prior_host(data.data, n_epochs, n_init=20)
                self._save("prior")
        self._engine.reset_optimizer(self._prior_lr)
        min_loss = float("inf")
        for _ in range(n_epochs):
            loss = self._pretrain_epoch(sess, data, "prior")
            if loss <= min_loss:
                min_loss = loss
                self._save("prior")
        return min_loss

    def pretrain(self, session, data, n_epochs_vae, n_epochs_gmm):
        """base_models.py:416-423."""
        assert(self.vae_train_step is not None and self.prior_train_step is not None)
        self.pretrain_vae(session, data, n_epochs_vae)
        self.pretrain_prior(session, data, n_epochs_gmm)
        # the main optimizer (define_train_step) is its own AdamOptimizer: fresh slots, its own learning rate
        self._engine.reset_optimizer(getattr(self, "_lr", None))

    # ------------------------------------------------------------------ checkpoint (trainables only, like tf.train.Saver)
    def state_dict(self):
        return {k: v for k, v in self._engine.get_parameters().items()}

    def load_state_dict(self, sd):
        self._engine.set_parameters(sd)


class VaDE(DeepMixtureVAE):
    """code/base_models.py:435-670 on the same HIP kernels: one encoder of FullyConnected layers
    784 -> 2000 -> 500 -> 500 (:490-499), mean / log_var linear straight off it (:501-507), q(c|x) := p(c|z) =
    get_cluster_probs(Z) (:526-527, priors.py:91-102) as the mixture weights of the exact KL and as the probabilities of
    the categorical KL, decoder D -> 500 -> 500 -> 2000 -> input (:530-547).  The per-batch step is the DMVAE step plan
    with dmvae_config.model = DMVAE_MODEL_VADE: no head hidden layers / logits, latent stage = dmvae_latent_fwd mode 2
    (csrc/latent_vade.hip), whose gradients include the path through the responsibilities into Z and the prior tables.
    cnn=True (:456-488): the batch as 28x28x1 images through the same six-convolution / three-pool stack as DMVAE's
    checked-in encoder, ending in ("fc", 2048 -> 128), with mean / log_var straight off those 128 units
    (dmvae_config.trunk = DMVAE_TRUNK_CNN, enc = (128,))."""

    _metrics_draws = 10                                     # get_cluster_metrics: get_accuracy's default k

    def __init__(self, name, input_type, input_dim, latent_dim, n_classes, activation=None, initializer=None, cnn=False, *,
                 batch_size=100, dtype="bf16", enc_layers=(2000, 500, 500), dec_layers=(500, 500, 2000), noise="device", seed=0,
                 deterministic=True, session=None, gmm="host", eval="host", gmm_seeding="host", label_weight=None):
        if label_weight is not None:
            raise NotImplementedError("VaDE(label_weight=...): VaDE's q(c|x) is p(c|z) -- a gradient on it runs through Z into the VaDE "
                                      "latent stage, which has no such input")
        if cnn and tuple(enc_layers) == (2000, 500, 500):
            enc_layers = (128,)            # base_models.py:486: ("fc", {"input_dim": 2048, "output_dim": 128})
        DeepMixtureVAE.__init__(self, name, input_type, input_dim, latent_dim, n_classes, activation=activation, initializer=initializer,
                                cnn=cnn, batch_size=batch_size, dtype=dtype, enc_layers=enc_layers, head_dim=64, dec_layers=dec_layers,
                                gumbel=False, temperature=1.0, noise=noise, seed=seed, deterministic=deterministic, session=session, gmm=gmm,
                                eval=eval, gmm_seeding=gmm_seeding)

    def build_graph(self):
        from dmvae_hip import StepEngine, default_session
        sess = self._session or default_session()
        self._session = sess
        enc_spec, prev = [], self.input_dim                   # the two DeepNetwork spec lists exactly as the reference writes them
        for w in self.enc_layers:
            enc_spec.append(("fc", {"input_dim": prev, "output_dim": w}))
            prev = w
        dec_spec, prev = [], self.latent_dim
        for w in self.dec_layers:
            dec_spec.append(("fc", {"input_dim": prev, "output_dim": w}))
            prev = w
        self.encoder_network = (_cnn_encoder_network(self.enc_layers[0]) if self.cnn else
                                DeepNetwork("layers", enc_spec, activation="relu", initializer="xavier"))
        self.decoder_network = DeepNetwork("layers", dec_spec, activation="relu", initializer="xavier")
        self._engine = StepEngine(self.input_dim, self.latent_dim, self.n_classes, enc_layers=self.enc_layers, head_dim=64,
                                  dec_layers=self.dec_layers, input_type=self.input_type, dtype=self.dtype, max_batch=self.batch_size,
                                  mode="exact", seed=self.seed + 7919 * sess.rank, deterministic=self.deterministic, session=sess,
                                  model="vade", cnn=self.cnn)
        self._engine.init_parameters(self.seed)
        self.X, self.epsilon = "X", "epsilon"
        self.mean, self.log_var, self.cluster_probs, self.Z = "mean", "log_var", "cluster_probs", "Z"
        self.decoded_X, self.reconstructed_X = "decoded_X", "reconstructed_X"
        self.latent_variables = dict()
        self.latent_variables.update({
            "Z": (priors.NormalMixtureFactorial("representation", self.latent_dim, self.n_classes, engine=self._engine), self.epsilon,
                  {"mean": self.mean, "log_var": self.log_var, "cluster_sample": False, "weights": self.cluster_probs}),
        })
        self.latent_variables.update({
            "C": (priors.DiscreteFactorial("cluster", 1, self.n_classes), None, {"probs": self.cluster_probs}),
        })
        return self

    def encode(self, X):
        """(mean, log_var) of q(z|x), base_models.py:501-507 (VaDE has no logits: q(c|x) comes from the sample)."""
        mean, log_var, _ = DeepMixtureVAE.encode(self, X)
        return mean, log_var

    def reconstruct(self, X, epsilon=None):
        mean, log_var = self.encode(X)
        Z = mean if epsilon is None else mean + np.exp(log_var / 2) * np.asarray(epsilon)
        return self.decode(Z)

    def cluster_probabilities(self, X, epsilon):
        """fetching `cluster_probs` with X and epsilon fed (base_models.py:659-663)"""
        mean, log_var = self.encode(X)
        Z = mean + np.exp(log_var / 2) * np.asarray(epsilon, dtype=np.float32)
        return self.latent_variables["Z"][0].get_cluster_probs(Z)

    # ------------------------------------------------------------------ pretraining (base_models.py:573-652)
    def define_pretrain_step(self, vae_lr, _prior_lr=None):
        self.define_train_loss()
        self.vae_loss = "recon"
        self._vae_lr, self._prior_lr = float(vae_lr), None
        self.vae_train_step = "adam_tf(recon_loss)"
        self.prior_train_step = None

    def pretrain_prior(self, session, data, n_epochs):
        """base_models.py:611-646: only the GMM initialisation of the prior tables (n_init = 5), no Adam stage."""
        if not self._restore("prior"):
            print("Could not load pretrained prior parameters")
            if n_epochs > 0 and self.gmm == "device":
                self._fit_prior_on_device(data.data, n_epochs, n_init=5)
                self._save("prior")
            elif n_epochs > 0:
                self._fit_prior_host(data.data, n_epochs, n_init=5)
                self._save("prior")

    def pretrain(self, session, data, n_epochs_vae, n_epochs_prior):
        assert(self.vae_train_step is not None)
        self.pretrain_vae(session, data, n_epochs_vae)
        self.pretrain_prior(session, data, n_epochs_prior)
        self._engine.reset_optimizer(getattr(self, "_lr", None))

    def get_accuracy(self, session, data, k=10):
        """base_models.py:654-670: cluster_probs averaged over k noise draws (the reference's NumPy stream, one
        sample_reparametrization_variables(n, ["Z"]) per draw over the whole set), then the clustering accuracy.
        eval="device": the encoder runs ONCE over the resident rows and the k draws, their responsibilities, the average and
        its arg-max are one kernel per batch (StepEngine.eval_clusters).  With noise="host" the k draws come from the same
        calls in the same order as below and are uploaded: the global NumPy stream ends where the host path leaves it, and the
        two accuracies differ only on rows whose two largest averaged responsibilities tie to float32 rounding.  With
        noise="device" the draws are Philox in the kernel (keyed by the plan seed, the count of evaluations of this model, the
        draw and the row's position): ANOTHER Monte-Carlo estimate than the host path's, and no NumPy draw is consumed, so a
        run's later shuffles differ from an eval="host" run's."""
        if self.eval == "device":
            import torch
            order, eps = data.order, None
            N, b = len(order), self._engine.max_batch
            if self.noise == "host":
                E = np.stack([np.asarray(self.sample_reparametrization_variables(N, variables=["Z"])[self.epsilon], dtype=np.float32)
                              for _ in range(k)])                                # [k, N, D], then batch after batch [k, n, D]
                eps = torch.as_tensor(np.concatenate([E[:, s:s + b].reshape(-1) for s in range(0, N, b)])).to(self._session.device)
            self._eval_calls += 1
            d = self._device_confusion(data, order, self.n_classes, draws=k, eps=eps, counter=self._eval_calls)
            return accuracy_from_confusion(d, N)
        X = data.data
        weights = []
        for _ in range(k):
            feed = self.sample_reparametrization_variables(len(X), variables=["Z"])
            weights.append(self.cluster_probabilities(X, feed[self.epsilon]))
        weights = np.mean(np.array(weights), axis=0)
        return get_clustering_accuracy(weights, data.classes)
