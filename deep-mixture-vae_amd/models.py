"""MoE / DeepMoE / DeepVariationalMoE -- drop-in for the class surface of code/models.py of the reference: a supervised
mixture of experts whose gate is the DMVAE's q(c|x) = softmax(logits).  The experts, the mixture, the loss and their gradients
run inside the DMVAE training step on the GPU (dmvae_plan_attach_moe: csrc/moe_head.hip, one more GEMM problem forward and one
more weight-gradient problem in the grouped dW + Adam launch).

Parameters: regression_weights [E, O, in] ~ N(0, 1) and regression_biases [O, E] = 0 (models.py:51-70).  The weights are drawn
by StepEngine.init_parameters from the same NumPy RandomState(seed) as the VAE's tensors, after the prior means (TF's own stream
is not reproduced, as for every other initialiser here)."""
import numpy as np

import base_models
from includes.utils import accuracy_from_confusion, get_moe_clustering_accuracy


class MoE:
    def __init__(self, name, input_type, input_dim, latent_dim, output_dim, n_experts, classification, activation=None, initializer=None,
                 lossVAE=1, featLearn=1, cnn=False, *, batch_size=100, dtype="bf16", enc_layers=(500, 500), head_dim=2000,
                 dec_layers=(2000, 500, 500), gumbel=False, temperature=1.0, noise="device", seed=0, session=None, eval="host"):
        if cnn:
            raise NotImplementedError("MoE with the CNN trunk: the flat input the experts read (featLearn off) is not resident in conv plans")
        if eval not in ("host", "device"):
            raise ValueError("eval must be 'host' or 'device'")
        self.eval = eval
        self.name = name
        self.input_dim, self.latent_dim, self.output_dim = int(input_dim), int(latent_dim), int(output_dim)
        self.input_type = input_type
        self.classification = bool(classification)
        self.n_experts = self.n_classes = int(n_experts)
        self.activation, self.initializer = activation, initializer
        self.vae = None
        self.featLearn = bool(featLearn)
        self.lossVAE = bool(lossVAE)
        self.cnn = False
        self._vae_kw = dict(batch_size=batch_size, dtype=dtype, enc_layers=enc_layers, head_dim=head_dim, dec_layers=dec_layers,
                            gumbel=gumbel, temperature=temperature, noise=noise, seed=seed, session=session)
        self.train_step = None
        self._replay, self._replay_key, self._perm = None, None, None

    def _define_vae(self):
        raise NotImplementedError

    def define_vae(self):
        self._define_vae()

    def build_graph(self):
        import torch
        from dmvae_hip import default_session
        sess = self._vae_kw["session"] or default_session()
        self._vae_kw["session"] = sess
        self.define_vae()
        # placeholder labels until a dataset is bound (train_op / get_accuracy point the plan at the dataset's device labels)
        self._labels0 = torch.zeros((1, self.output_dim), dtype=torch.float32, device=sess.device)
        self.vae._moe_spec = dict(n_experts=self.n_experts, output_dim=self.output_dim, featLearn=self.featLearn,
                                  classification=self.classification, lossVAE=self.lossVAE, labels=self._labels0)
        self.vae.build_graph()
        self.X, self.Z, self.Y = self.vae.X, self.vae.Z, "Y"
        self.reconstructed_X = self.vae.reconstructed_X
        self.expert_probs = self.vae.cluster_probs
        self.reconstructed_Y, self.reconstructed_Y_soft = "reconstructed_Y", "reconstructed_Y_soft"
        self.regression_weights, self.regression_biases = "regression_weights", "regression_biases"
        return self

    @property
    def engine(self):
        return self.vae.engine

    def sample_generative_feed(self, n, **kwargs):
        return self.vae.sample_generative_feed(n, **kwargs)

    def sample_reparametrization_variables(self, n):
        return self.vae.sample_reparametrization_variables(n)

    def define_train_loss(self):
        self.vae.define_train_loss()
        self.recon_loss = "loss_moe (moe_head.hip)"
        self.loss = "loss_moe + vae.loss" if self.lossVAE else "loss_moe"

    def define_pretrain_step(self, *a, **k):
        raise NotImplementedError("--pretrain with a MoE model is not built")

    def define_train_step(self, init_lr, decay_steps, decay_rate=0.9, pretrain_init_lr=None, pretrain_decay_steps=None, pretrain_decay_rate=None):
        """models.py:165-181: one AdamOptimizer minimising loss (constant learning rate: global_step is the literal 0)"""
        self.define_train_loss()
        self.vae.define_train_step(init_lr, decay_steps, decay_rate)
        self.train_step = "adam_tf"

    def _bind(self, data):
        import torch
        sess = self.vae._session
        if sess.world_size > 1:
            raise NotImplementedError("MoE models train on one rank")
        eng = self.engine
        rows, labels = data.device_rows(sess.device), data.device_labels(sess.device)
        eng.moe_set_labels(labels)
        order = data.reshuffle()
        t = torch.as_tensor(np.ascontiguousarray(order, dtype=np.int32))
        if self._perm is None or self._perm.numel() != t.numel():
            self._perm = torch.empty(t.numel(), dtype=torch.int32, device=sess.device)
        self._perm.copy_(t)
        return rows, labels, self._perm, order

    def train_op(self, session, data, kl_ratio=1.0):
        """models.py:194-221: one epoch over MEDataset.get_batches(); returns (sum batch_loss / epoch_len, batch_acc of the LAST
        batch, sum loss_moe / epoch_len).  Losses accumulate on the device and are read once per epoch."""
        assert self.train_step is not None
        import torch
        eng = self.engine
        b = eng.max_batch
        if data.batch_size != b:
            raise ValueError("batch_size %d != the size the model was built for (%d)" % (data.batch_size, b))
        rows, labels, perm, _ = self._bind(data)
        n_full, tail = divmod(data.len, b)
        eng.reset_epoch(n_full + (1 if tail else 0), kl_ratio=kl_ratio, epoch_weight=1.0 / data.epoch_len)

        def host_feed(n):
            feed = self.sample_reparametrization_variables(n)        # C first, then Z: the reference's order
            eps = torch.as_tensor(np.ascontiguousarray(feed[self.vae.epsilon], dtype=np.float32)).to(eng.device)
            g = None
            if self.vae.gumbel:
                g = torch.as_tensor(np.ascontiguousarray(feed[self.vae.cluster].reshape(n, self.n_experts), dtype=np.float32)).to(eng.device)
            return eps, g

        if self.vae.noise == "host":
            eng.moe_zero_acc()
            for i in range(n_full):
                eps, g = host_feed(b)
                eng.train_step(rows, perm, b, eps, g, first=i * b)
        else:
            key = (rows.data_ptr(), labels.data_ptr(), perm.data_ptr(), b)
            if n_full > 0 and (self._replay is None or self._replay_key != key):
                self._replay = eng.capture_step(rows, perm)
                self._replay_key = key
                eng.reset_epoch(n_full + (1 if tail else 0), kl_ratio=kl_ratio, epoch_weight=1.0 / data.epoch_len)
            eng.moe_zero_acc()
            for _ in range(n_full):
                self._replay()
        last = b
        if tail:
            eps, g = host_feed(tail) if self.vae.noise == "host" else (None, None)
            eng.train_step(rows, perm, tail, eps, g, first=n_full * b, inv_B=1.0 / tail)
            last = tail
        torch.cuda.synchronize(eng.device)
        acc = eng.moe_acc()
        st = eng.read_state()
        loss_cls = float(acc[0]) / data.epoch_len
        loss = loss_cls + (float(st.epoch_loss) if self.lossVAE else 0.0)
        batch_error = float(acc[3])
        batch_acc = 1 - batch_error / last if self.classification else -batch_error
        self.last_epoch = dict(loss=loss, loss_moe=loss_cls, batch_acc=batch_acc, kl_ratio=float(kl_ratio), rows=int(data.len))
        return loss, batch_acc, loss_cls

    def get_accuracy(self, session, data):
        """models.py:115-135: (1 - errors / len, clustering accuracy) for classification, (-sum error / epoch_len, clustering
        accuracy) for regression.  The clustering accuracy sizes its matrix max(E, n_classes): see get_moe_clustering_accuracy.
        eval="device": the gate's arg-max and the confusion matrix are taken on the GPU behind every moe_predict
        (StepEngine.confusion_add on the "logits" view) instead of copying each batch's logits to the host; the same matrix."""
        import torch
        eng = self.engine
        rows, labels, perm, order = self._bind(data)
        eng.moe_zero_acc()
        b = eng.max_batch
        n_classes = int(np.max(data._cls)) + 1
        device = self.eval == "device"
        if device:
            cls_d = data.device_classes(eng.device)
            conf = eng.confusion_buffer(max(self.n_experts, n_classes), eng.device)
        logits = []
        for s in range(0, data.len, b):
            n = min(b, data.len - s)
            eng.load_batch(rows, perm, s, n)
            eng.moe_predict(n)
            if device:
                eng.confusion_add(conf, eng.view("logits", n), cls_d, perm, s, n)
            else:
                logits.append(eng.view("logits", n).cpu().numpy().copy())
        torch.cuda.synchronize(eng.device)
        error = float(eng.moe_acc()[1])
        if device:
            acc_cl = accuracy_from_confusion(eng.read_confusion(conf), data.len)
        else:
            acc_cl = get_moe_clustering_accuracy(np.concatenate(logits, axis=0), data._cls[order], n_classes)
        if self.classification:
            return 1 - error / data.len, acc_cl
        return -error / data.epoch_len, acc_cl

    def get_augmentation_consistency(self, session, data, augment, n_draws=4, seed=0, counter=0):
        raise NotImplementedError("get_augmentation_consistency with %s: the MoE data set carries regression labels that are functions of the "
                                  "grey rows, and a warped row has none; the evaluator is built for DeepMixtureVAE and VaDE" % type(self).__name__)

    def get_cluster_metrics(self, session, data, silhouette=True, counter=0, return_labels=False):
        """The gate's cluster quality (DeepMixtureVAE.get_cluster_metrics): dict(acc, nmi, ari, purity, silhouette, n_clusters_used)
        of the experts' arg-max against the classes, the matrix sized max(E, n_classes) as get_accuracy sizes it.  No reshuffle."""
        n_classes = int(np.max(data._cls)) + 1
        return self.vae._cluster_metrics(data, max(self.n_experts, n_classes), silhouette, counter, return_labels)

    def get_knn_accuracy(self, session, train_data, test_data, k=10, return_confusion=False):
        """kNN accuracy of the gate's encoder means (DeepMixtureVAE.get_knn_accuracy).  No reshuffle."""
        return self.vae.get_knn_accuracy(session, train_data, test_data, k=k, return_confusion=return_confusion)

    def get_linear_probe_accuracy(self, session, train_data, test_data, C=1.0, tol=1e-4, max_iter=200, standardize=True, return_confusion=False):
        """Linear-probe accuracy of the gate's encoder means (DeepMixtureVAE.get_linear_probe_accuracy).  No reshuffle."""
        res = self.vae.get_linear_probe_accuracy(session, train_data, test_data, C=C, tol=tol, max_iter=max_iter, standardize=standardize,
                                                 return_confusion=return_confusion)
        self.last_linear_probe_ = self.vae.last_linear_probe_
        return res

    def get_few_label_accuracy(self, session, train_data, test_data, n_labeled=100, seed=0, k=7, alpha=0.8, weights="connectivity", labeled=None):
        """Few-label accuracy of the gate's encoder means by label spreading (DeepMixtureVAE.get_few_label_accuracy).  No reshuffle."""
        if self.vae is None:
            raise NotImplementedError("get_few_label_accuracy: %s has no encoder to take latent means from" % type(self).__name__)
        res = self.vae.get_few_label_accuracy(session, train_data, test_data, n_labeled=n_labeled, seed=seed, k=k, alpha=alpha, weights=weights,
                                              labeled=labeled)
        self.last_label_spreading_ = self.vae.last_label_spreading_
        return res

    def get_latent_map(self, session, data, perplexity=30.0, n_iter=1000, method="auto", trust_neighbors=5, counter=0):
        """The t-SNE map of the gate's encoder means with the classes and the experts' arg-max (DeepMixtureVAE.get_latent_map), the
        label matrix sized max(E, n_classes) as get_cluster_metrics sizes it.  No reshuffle."""
        n_classes = int(np.max(data._cls)) + 1
        return self.vae._latent_map(data, max(self.n_experts, n_classes), perplexity, n_iter, method, trust_neighbors, counter)

    def get_sample_quality(self, session, data, k=5, n_samples=None, space="latent", counter=0):
        """Precision, recall, density and coverage of the gate's decoded prior samples (DeepMixtureVAE.get_sample_quality).  No reshuffle."""
        return self.vae.get_sample_quality(session, data, k=k, n_samples=n_samples, space=space, counter=counter)

    def get_sample_distance(self, session, data, eps_rel=0.05, n_samples=None, space="latent", counter=0, tol=1e-4, max_iter=500):
        """Sinkhorn divergence between the gate's decoded prior samples and the data (DeepMixtureVAE.get_sample_distance).  No reshuffle."""
        return self.vae.get_sample_distance(session, data, eps_rel=eps_rel, n_samples=n_samples, space=space, counter=counter, tol=tol,
                                            max_iter=max_iter)

    def get_reconstruction_quality(self, session, data, image_shape=None, n_worst=10, **kw):
        """SSIM, PSNR and MSE of the gate's reconstructions, per class, with the worst rows (DeepMixtureVAE.get_reconstruction_quality).
        No reshuffle."""
        return self.vae.get_reconstruction_quality(session, data, image_shape=image_shape, n_worst=n_worst, **kw)

    def get_sample_diversity(self, session, n_per_cluster=32, image_shape=None, counter=0, **kw):
        """Mean pairwise SSIM among the gate's decoded prior samples, within and between components (DeepMixtureVAE.get_sample_diversity)."""
        return self.vae.get_sample_diversity(session, n_per_cluster=n_per_cluster, image_shape=image_shape, counter=counter, **kw)

    def get_cluster_exemplars(self, session, data, n=10):
        """The rows of `data` nearest each expert's prior mean (DeepMixtureVAE.get_cluster_exemplars).  No reshuffle."""
        return self.vae.get_cluster_exemplars(session, data, n=n)

    def predict(self, X):
        """(reconstructed_Y, reconstructed_Y_soft) of models.py:83-108 for the rows X (regression: the prediction twice)"""
        import torch
        eng = self.engine
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        b = eng.max_batch
        out = []
        for s in range(0, len(X), b):
            xb = torch.as_tensor(X[s:s + b]).to(eng.device)
            n = xb.shape[0]
            eng.load_batch(xb, None, 0, n)
            eng.moe_predict(n)
            out.append(eng.view("moe_pred", n).cpu().numpy().astype(np.float64))
        soft = np.concatenate(out, axis=0)
        if not self.classification:
            return soft, soft
        return np.eye(self.output_dim)[np.argmax(soft, axis=1)], soft

    def state_dict(self):
        """the trainables; the experts also under the reference's names and shapes"""
        sd = self.vae.state_dict()
        w, bias = self.engine.moe_reference_parameters()
        sd.pop("W_moe"), sd.pop("b_moe")
        sd["regression_weights"], sd["regression_biases"] = w, bias
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        w = np.asarray(sd.pop("regression_weights"))
        bias = np.asarray(sd.pop("regression_biases"))
        E, O_, n_in = w.shape
        sd["W_moe"] = w.transpose(2, 0, 1).reshape(n_in, E * O_)
        sd["b_moe"] = bias.T.reshape(E * O_)
        self.vae.load_state_dict(sd)


class DeepMoE(MoE):
    """models.py:239-250: gate = a DeepMixtureVAE with latent_dim = 1, lossVAE = 0 (the VAE terms contribute no gradient)"""
    def __init__(self, name, input_type, input_dim, output_dim, n_experts, classification, activation=None, initializer=None, featLearn=0,
                 cnn=False, **kw):
        MoE.__init__(self, name, input_type, input_dim, 1, output_dim, n_experts, classification, activation=activation,
                     initializer=initializer, lossVAE=0, featLearn=featLearn, cnn=cnn, **kw)

    def _define_vae(self):
        self.vae = base_models.DeepMixtureVAE("null_vae", self.input_type, self.input_dim, self.latent_dim, self.n_experts,
                                              activation=self.activation, initializer=self.initializer, **self._vae_kw)


class DeepVariationalMoE(MoE):
    """models.py:252-262: gate = a DeepMixtureVAE of latent_dim, loss = loss_moe + vae.loss"""
    def __init__(self, name, input_type, input_dim, latent_dim, output_dim, n_experts, classification, activation=None, initializer=None,
                 featLearn=1, cnn=False, **kw):
        MoE.__init__(self, name, input_type, input_dim, latent_dim, output_dim, n_experts, classification, activation=activation,
                     initializer=initializer, featLearn=featLearn, cnn=cnn, **kw)

    def _define_vae(self):
        self.vae = base_models.DeepMixtureVAE("deep_mixture_vae", self.input_type, self.input_dim, self.latent_dim, self.n_experts,
                                              activation=self.activation, initializer=self.initializer, **self._vae_kw)


class VaDEMoE(MoE):
    def __init__(self, *a, **k):
        raise NotImplementedError("VaDEMoE: its gate p(c|z) sends the MoE gradients through Z into the VaDE latent stage "
                                  "(latent_vade.hip), which has no such input")
