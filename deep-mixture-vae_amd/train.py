"""Training CLI of the DMVAE drop-in -- same flags and flow as code/train.py of
the reference (argparse :28-97, main :101-338) for --model dmvae, with the
per-batch path on MI355X.  Run from this directory:  python train.py [flags]
Multi-GPU (one process per GPU, RCCL gradient all-reduce):
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py --batch_size 32768
(with more than one rank only full global batches are trained: the batch must not exceed the row count)
Flags that the reference accepts but that address models outside the DMVAE hot
path (--model dmoe/dvmoe/vademoe, --visdom) are parsed and rejected /
ignored with a message, see SURVEY.md 2.1.  --plotting writes the reference's
two figures (regenerated.png, sampled.png) as PNG grids.  --pretrain runs the two
pretraining stages of base_models.py:304-423 (recon-only Adam at epsilon = 0,
GMM-initialised prior tables, latent-loss Adam over the c-head).
New flags (defaults = reference behaviour): --batch_size, --dtype, --seed,
--host_noise, --gumbel, --temperature, --enc_layers, --head_dim, --dec_layers,
--gmm, --gmm_seeding (host | device: where --gmm device draws its k-means++ centres),
--eval (host | device: where get_accuracy takes its arg-max and confusion matrix),
--loglik S (dmvae / vade: held-out log-likelihood of the test set per epoch, the importance-weighted bound with S draws; 0 = off),
--metrics (per epoch: NMI, ARI, purity and the silhouette coefficient of the test set's latent means beside the accuracy, get_cluster_metrics),
--diagnostics (dmvae / vade, per epoch on the test set: the estimate of I(x;z), KL(q(z) || p(z)) and the active units, get_posterior_diagnostics),
--knn K (per epoch: the accuracy of a K-nearest-neighbour vote among the train split's latent means on the test set's, get_knn_accuracy; 0 = off),
--probe / --probe_C (per epoch: the accuracy on the test set of a linear probe -- multinomial logistic regression, inverse penalty probe_C --
fitted on the train split's latent means, get_linear_probe_accuracy),
--few_label L / --few_label_seed (per epoch: the test accuracy of label spreading over the nearest-neighbour graph of the train split's and the
test set's latent means from L stratified labels of the train split, get_few_label_accuracy; 0 = off),
--sample_quality K (per epoch on the test set: improved precision / recall and density / coverage of the decoded draws from the mixture prior,
K-th-neighbour balls, per prior component and per class, get_sample_quality; 0 = off),
--sample_distance (per epoch on the test set: the Sinkhorn divergence between the decoded draws from the mixture prior and the data, per prior
component and per class, get_sample_distance),
--recon_quality (per epoch on the test set: SSIM, PSNR and MSE of the reconstructions, per class, get_reconstruction_quality),
--sample_diversity N (per epoch: the mean pairwise SSIM among N decoded prior draws per mixture component, within and between components,
get_sample_diversity; 0 = off),
--latent_map (off | auto | exact | knn: with --plotting, latent.png -- the t-SNE map of the encoder means coloured by class and by cluster,
get_latent_map -- of the test set at the plot epochs and of the whole train set at the end, lmTrust / lmKL in that epoch's JSONL record; knn is
the kNN-sparse P with exact repulsion, dmvae_hip.tsne.TSNE(method="knn"), which "auto" takes above 32768 rows),
--tsne (off | host | device: with --plotting, sampled.png gains the t-SNE scatter of the prior samples, embedded by sklearn on the CPU or by
the exact t-SNE in HIP, dmvae_hip.tsne.TSNE),
--binarize (off | static | dynamic | threshold; dmvae / vade: train and evaluate on binarised pixels, drawn on the device -- static: one Bernoulli
draw of every row; dynamic: a fresh draw of the train set per epoch, the test set and the --knn / --probe split static; threshold: x > 0.5 --
so that llTest is a Bernoulli log-likelihood in nats, comparable with the literature's binarised-MNIST figures; off = the reference's grey
levels as soft targets) and --binarize_seed (the key of the draws, the same on every rank),
--augment SPEC / --augment_seed S (dmvae / vade: every epoch trains on a fresh random affine warp of every train row, drawn and applied on the
device -- SPEC e.g. rotate=10,translate=2,scale=0.9:1.1,shear=5 in degrees, pixels and factors; the test set and every evaluation stay clean;
off by default) and --aug_consistency SPEC / --aug_draws J (per epoch on the test set: augAgree, the share of rows that keep their cluster
under J random warps of SPEC, and the accuracy of the warped rows under the clean matching, get_augmentation_consistency),
--n_labeled L / --label_weight A / --label_seed S (dmvae, one rank: semi-supervised training -- L rows of the train split, stratified by
class, keep their label and every step adds A * N / L * the cross-entropy of q(c|x) = softmax(logits) on the labelled rows of its batch
(csrc/label_xent.hip), which pulls cluster c onto class c; the epoch line gains accDirect, the share of test rows whose arg-max cluster IS
their class (get_direct_accuracy), the JSONL acc_direct_test, label_xent, label_rows, label_acc, n_labeled, label_weight; 0 = off, and then
the plan and the run are what they were; refused with --model vade | dmoe | dvmoe and with more than one rank).
"""
import argparse
import json
import math
import os
import sys
import time
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

parser = argparse.ArgumentParser(description="DMVAE training on MI355X (flag names and defaults of the reference's train.py:28-97)")

# (flag, type, default, what it does here).  Names and defaults are the reference's CLI contract; the
# descriptions say what THIS implementation does with each flag.
_FLAGS = [
    ("model", str, "dmvae", "model family: dmvae, vade, dmoe (DeepMoE) or dvmoe (DeepVariationalMoE); vademoe is not built"),
    ("model_name", str, "", "directory name under saved-models/<dataset>/ (default: the model family)"),
    ("dataset", str, "mnist", "mnist | fashion-mnist | synthetic (idx files under data/<dataset>/, else a synthetic stand-in)"),
    ("latent_dim", int, 10, "width D of the Gaussian latent z"),
    ("output_dim", int, 1, "MoE regression target width (classification: the dataset's class count)"),
    ("n_clusters", int, -1, "mixture components K; -1 takes the dataset's class count"),
    ("n_experts", int, 5, "MoE expert count (= the gate's clusters)"),
    ("n_epochs", int, 500, "training epochs"),
    ("pretrain_epochs_vae", int, 200, "epochs of the reconstruction-only pretraining stage"),
    ("pretrain_epochs_prior", int, 200, "epochs of the prior stage (also max_iter of the GMM that seeds the prior tables)"),
    ("init_lr", float, 0.002, "Adam learning rate (constant: the reference's decay is a no-op, SURVEY F3)"),
    ("decay_rate", float, 0.9, "accepted and inert, as in the reference (global_step is the literal 0)"),
    ("decay_epochs", int, 25, "accepted and inert, see --decay_rate"),
    ("pretrain_vae_lr", float, 0.0005, "Adam learning rate of the reconstruction-only stage"),
    ("pretrain_decay_rate", float, 0.9, "accepted and inert"),
    ("pretrain_decay_epochs", int, 25, "accepted and inert"),
    ("pretrain_prior_lr", float, 0.0005, "Adam learning rate of the prior stage"),
    ("anneal_step", float, 0.1, "increment of the KL weight at each annealing point"),
    ("anneal_epochs", int, 1000, "epochs between two increments of the KL weight"),
    ("plot_epochs", int, 100, "epochs between two sets of sample / reconstruction grids"),
    ("save_epochs", int, 10, "epochs between two --debug stops"),
]
_SWITCHES = [
    ("classification", "MoE objective: classification (one-hot class labels) instead of regression"),
    ("pretrain", "run the two pretraining stages before training"),
    ("kl_annealing", "start the KL weight at 0 and raise it by --anneal_step every --anneal_epochs"),
    ("plotting", "write sampled.png / regenerated.png grids every --plot_epochs"),
    ("debug", "stop in pdb on the first batch every --save_epochs"),
    ("visdom", "accepted; no Visdom server is contacted"),
    ("featLearn", "MoE experts read relu(mean) of the gate's VAE instead of X"),
]
for _name, _type, _default, _help in _FLAGS:
    parser.add_argument("--" + _name, type=_type, default=_default, help=_help)
for _name, _help in _SWITCHES:
    parser.add_argument("--" + _name, action="store_true", default=False, help=_help)
# ---- extensions (defaults reproduce the reference)
parser.add_argument("--batch_size", type=int, default=100, help="GLOBAL batch size (reference hard-codes 100, train.py:215-216)")
parser.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="bf16 MFMA (throughput) or exact fp32 (parity)")
parser.add_argument("--seed", type=int, default=0)
parser.add_argument("--host_noise", action="store_true", default=False,
                    help="draw epsilon / gumbel on the host from NumPy like the reference instead of on-device Philox")
parser.add_argument("--gumbel", action="store_true", default=False, help="Gumbel-Softmax relaxed KL (report's variant; off = checked-in graph)")
parser.add_argument("--temperature", type=float, default=1.0)
parser.add_argument("--enc_layers", type=str, default="500,500")
parser.add_argument("--head_dim", type=int, default=2000)
parser.add_argument("--dec_layers", type=str, default="2000,500,500")
parser.add_argument("--gmm", type=str, default="host", choices=["host", "device"],
                    help="--pretrain: fit the prior tables' Gaussian mixture with sklearn on the host (the reference) or with dmvae_hip.gmm.DiagGMM on the device")
parser.add_argument("--gmm_seeding", type=str, default="host", choices=["host", "device"],
                    help="--gmm device: k-means++ seeding in NumPy on a host copy of the encoder means, or on the device (dmvae_gmm_seed)")
parser.add_argument("--eval", type=str, default="host", choices=["host", "device"],
                    help="get_accuracy: arg-max and confusion matrix in NumPy from scores copied back per batch (the reference's way) or on the "
                         "device from the resident rows (one small matrix read back per call)")
parser.add_argument("--loglik", type=int, default=0,
                    help="dmvae / vade: S > 0 adds llTest to the epoch line -- the test set's log-likelihood in nats per row, the importance-weighted "
                         "bound with S draws computed on the device (get_log_likelihood); 0 = off")
parser.add_argument("--metrics", action="store_true", default=False,
                    help="per epoch, beside the accuracy: NMI, ARI and purity of the test set's clusters against its classes and the silhouette "
                         "coefficient of its latent means, computed on the device (get_cluster_metrics); adds nmiTest / silTest to the epoch line")
parser.add_argument("--diagnostics", action="store_true", default=False,
                    help="dmvae / vade, per epoch on the test set: how much of the KL term is information about x (miTest, at most log N), how much "
                         "is mismatch between the aggregate posterior and the mixture prior, and how many latent dimensions are active (auTest), "
                         "all pairs on the device (get_posterior_diagnostics); rank 0 alone evaluates")
parser.add_argument("--knn", type=int, default=0,
                    help="K > 0 adds knnTest to the epoch line -- are rows of one class close in latent space, whatever the clusters did with them: "
                         "the accuracy on the test set of a K-nearest-neighbour vote among the encoder means of the train split, all pairs on the "
                         "device (get_knn_accuracy); rank 0 alone evaluates; 0 = off")
parser.add_argument("--probe", action="store_true", default=False,
                    help="adds probeTest to the epoch line -- are the classes linearly separable in latent space: the accuracy on the test set of a "
                         "multinomial logistic regression fitted on the encoder means of the train split, loss and gradient on the device "
                         "(get_linear_probe_accuracy); rank 0 alone evaluates")
parser.add_argument("--probe_C", type=float, default=1.0, help="--probe: the inverse of the L2 penalty, as sklearn's C")
parser.add_argument("--few_label", type=int, default=0,
                    help="L > 0 adds flTest to the epoch line -- given this latent space and only L labels of the train split (stratified, "
                         "includes.utils.choose_labeled), how many test rows get the right class: label spreading over the nearest-neighbour "
                         "graph of the train split's and the test set's encoder means on the device (get_few_label_accuracy), with the "
                         "1-nearest-neighbour and linear-probe accuracies on the same L labels alone in the JSONL record; rank 0 alone "
                         "evaluates; 0 = off")
parser.add_argument("--few_label_seed", type=int, default=0,
                    help="--few_label: the seed of the stratified draw; the default is --label_seed's, so --n_labeled L --few_label L evaluates "
                         "with exactly the labels the training saw")
parser.add_argument("--sample_quality", type=int, default=0,
                    help="K > 0 adds precTest and covTest to the epoch line -- are the decoded draws from the mixture prior realistic, and do they "
                         "cover the test set: improved precision / recall and density / coverage with K-th-neighbour balls in the space of the "
                         "encoder means, per prior component and per class in the JSONL record, all pairs on the device (get_sample_quality); "
                         "rank 0 alone evaluates; 0 = off")
parser.add_argument("--sample_distance", action="store_true", default=False,
                    help="add sdTest to the epoch line -- how far the distribution of the decoded draws from the mixture prior is from the test "
                         "set's: the Sinkhorn divergence (debiased entropic optimal transport, squared Euclidean cost) between their encoder "
                         "means, with its split per prior component and per class in the JSONL record, all pairs on the device "
                         "(get_sample_distance); rank 0 alone evaluates")
parser.add_argument("--recon_quality", action="store_true", default=False,
                    help="add ssimTest and psnrTest to the epoch line -- the structural similarity (valid 11-tap Gaussian windows, centred moments) "
                         "and the PSNR of the test set's reconstructions -- and those, mseTest and the per-class vectors to the JSONL record, on "
                         "the device (get_reconstruction_quality); rank 0 alone evaluates")
parser.add_argument("--sample_diversity", type=int, default=0,
                    help="N > 0 adds divTest to the epoch line -- the mean pairwise SSIM among N decoded prior draws of one mixture component, "
                         "averaged over the components (near 1: a component generates one image) -- and the per-component vectors to the JSONL "
                         "record, on the device (get_sample_diversity); rank 0 alone evaluates; 0 = off")
parser.add_argument("--tsne", type=str, default="off", choices=["off", "host", "device"],
                    help="--plotting: add the t-SNE scatter of the prior samples (1000 per cluster) to sampled.png, embedded with sklearn on the "
                         "host (the reference's call) or with the exact t-SNE on the device (dmvae_hip.tsne.TSNE); off = the sample grid alone")
parser.add_argument("--latent_map", type=str, default="off", choices=["off", "auto", "exact", "knn"],
                    help="--plotting: write latent.png, the t-SNE map of the encoder means coloured by class and by cluster (get_latent_map) -- of "
                         "the test set at the plot epochs, of the whole train set at the end -- and add lmTrust / lmKL to that epoch's JSONL record; "
                         "exact: the dense P (up to 32768 rows), knn: P over the nearest rows with exact repulsion (dmvae_hip.tsne.TSNE("
                         "method=\"knn\")), auto: exact up to 32768 rows and knn above; rank 0 alone draws; off = no map")
parser.add_argument("--binarize", type=str, default="off", choices=["off", "static", "dynamic", "threshold"],
                    help="dmvae / vade: binarise the pixels on the device (Dataset(binarize=...)) -- static: one Bernoulli draw per row (a fixed "
                         "binarised data set); dynamic: the train set is redrawn every epoch, the test set and the --knn / --probe split keep one "
                         "draw (Salakhutdinov & Murray 2008; Burda et al. 2016); threshold: x > 0.5 -- so that llTest is the log-probability of "
                         "a binary data set in nats; off = grey levels as soft Bernoulli targets (the reference)")
parser.add_argument("--n_labeled", type=int, default=0,
                    help="dmvae, one rank: semi-supervised training -- this many rows of the TRAIN split keep their class (stratified, "
                         "includes.utils.choose_labeled) and a cross-entropy on q(c|x) pulls cluster c onto class c (csrc/label_xent.hip); 0 = off")
parser.add_argument("--label_weight", type=float, default=1.0,
                    help="--n_labeled: alpha, the weight of the mean cross-entropy of the labelled set against the per-row VAE loss")
parser.add_argument("--label_seed", type=int, default=0, help="--n_labeled: the seed of the stratified draw (its own RandomState)")
parser.add_argument("--augment", type=str, default=None, metavar="SPEC",
                    help="dmvae / vade: train every epoch on a fresh random affine warp of the train rows (Dataset(augment=...), csrc/augment.hip): "
                         "SPEC is rotate=DEG,translate=PX,scale=LO:HI,shear=DEG with any key left out; the rows are square images.  The test set, "
                         "the --knn / --probe split and every evaluator keep the clean rows.  Default: off.")
parser.add_argument("--augment_seed", type=int, default=0,
                    help="--augment: the seed of the draws (Philox stream 9); every rank of a data-parallel run uses this same value")
parser.add_argument("--aug_consistency", type=str, default=None, metavar="SPEC",
                    help="dmvae / vade: per epoch, the share of test rows whose cluster survives a random warp of SPEC (augAgree) and the accuracy "
                         "of the warped rows under the clean rows' matching (get_augmentation_consistency)")
parser.add_argument("--aug_draws", type=int, default=4, help="--aug_consistency: warps per row")
parser.add_argument("--binarize_seed", type=int, default=0,
                    help="--binarize: the seed of the draws (Philox stream 8); every rank of a data-parallel run uses this same value, not a "
                         "per-rank one: the ranks hold the whole data set and must agree on it")
parser.add_argument("--cnn", action="store_true", default=False,
                    help="the checked-in convolutional encoder trunk (base_models.py:156,176-216) instead of the MLP branch")


def _few_label_record(fl):
    """the JSONL keys of --few_label"""
    return dict(few_label_test=float(fl["accuracy"]), few_label_unlabeled_train=float(fl["accuracy_unlabeled_train"]), few_label_knn1=float(fl["knn1"]),
                few_label_probe=float(fl["probe"]), few_label_unreached=int(fl["n_unreached"]), few_label_iters=int(fl["n_iter"]),
                few_label_n=int(fl["n_labeled"]))


def _metrics_record(cm):
    """the JSONL keys of --metrics (a silhouette that is not defined -- fewer than two clusters in use -- is written as null)"""
    sil = float(cm["silhouette"])
    return dict(nmi_test=float(cm["nmi"]), ari_test=float(cm["ari"]), purity_test=float(cm["purity"]),
                silhouette_test=None if math.isnan(sil) else sil, clusters_used_test=int(cm["n_clusters_used"]))


def _diagnostics_record(pd):
    """the JSONL keys of --diagnostics"""
    return dict(mi_test=float(pd["mi"]), marginal_kl_test=float(pd["marginal_kl"]), rate_test=float(pd["rate"]), mi_cap_test=float(pd["mi_cap"]),
                active_units_test=int(pd["active_units"]))


def _sample_quality_record(sq):
    """the JSONL keys of --sample_quality (a class without rows is written as null)"""
    vec = lambda v: [None if math.isnan(x) else float(x) for x in v]
    rec = dict(precTest=float(sq["precision"]), recTest=float(sq["recall"]), denTest=float(sq["density"]), covTest=float(sq["coverage"]),
               sq_k=int(sq["k"]), sq_samples=int(sq["n_samples"]), precision_per_cluster=vec(sq["precision_per_cluster"]),
               density_per_cluster=vec(sq["density_per_cluster"]))
    if "coverage_per_class" in sq:
        rec.update(coverage_per_class=vec(sq["coverage_per_class"]), recall_per_class=vec(sq["recall_per_class"]))
    return rec


def _sample_distance_record(sk):
    """the JSONL keys of --sample_distance (a class without rows is written as null in its mean; the means stay out of the record)"""
    rec = dict(sdTest=float(sk["divergence"]), sd_eps=float(sk["eps"]), sd_iters=[int(n) for n in sk["n_iter"]], sd_err=[float(e) for e in sk["err"]],
               sd_per_cluster=[float(x) for x in sk["per_cluster"]])
    if "per_class" in sk:
        rec.update(sd_per_class=[float(x) for x in sk["per_class"]])
    return rec


def _ssim_record(rq, sd):
    """the JSONL keys of --recon_quality and --sample_diversity (nan, and the PSNR of an exact reconstruction, are written as null)"""
    num = lambda x: float(x) if math.isfinite(x) else None
    vec = lambda v: [num(x) for x in v]
    rec = {}
    if rq is not None:
        rec.update(ssimTest=float(rq["ssim"]), psnrTest=num(rq["psnr"]), mseTest=float(rq["mse"]), worst_rows_test=[int(i) for i in rq["worst"]])
        if "ssim_per_class" in rq:
            rec.update(ssim_per_class=vec(rq["ssim_per_class"]), mse_per_class=vec(rq["mse_per_class"]))
    if sd is not None:
        rec.update(divTest=float(np.mean(sd["ssim_within"])), div_n=int(sd["n_per_cluster"]), ssim_within=vec(sd["ssim_within"]),
                   ssim_between=num(sd["ssim_between"]), ssim_between_per_cluster=vec(sd["ssim_between_per_cluster"]),
                   collapsed=list(sd["collapsed"]))
    return rec


def main(argv):
    import torch
    import base_models
    from includes.utils import load_data, Dataset
    from includes import visualization
    from dmvae_hip import Session

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    np.random.seed(argv.seed)

    model_str, model_name = argv.model, argv.model_name
    if argv.n_labeled < 0:
        raise ValueError("--n_labeled must be >= 0")
    if argv.n_labeled > 0 and model_str != "dmvae":
        raise NotImplementedError("--n_labeled: the label term acts on DMVAE's q(c|x) = softmax(logits); VaDE's q(c|x) is p(c|z) (the gradient would "
                                  "run through Z into the VaDE latent stage) and the MoE models have their own supervised loss")
    if argv.n_labeled > 0 and world > 1:
        raise NotImplementedError("--n_labeled: the label term is built and tested on one rank")
    if model_str in ("dmoe", "dvmoe"):
        return main_moe(argv, world, rank)
    if model_str == "vademoe":
        raise NotImplementedError("--model vademoe: its gate p(c|z) sends gradients through Z into the VaDE latent stage (not built)")
    if model_str not in ("dmvae", "vade"):
        raise NotImplementedError
    plotting = argv.plotting and rank == 0 and argv.dataset == "mnist"   # train.py:157-163: plots exist for the image sets
    if argv.visdom and rank == 0:
        print("--visdom: accepted, not used")

    dataset = load_data(argv.dataset, classification=argv.classification, output_dim=argv.output_dim)
    if rank == 0:
        print(dataset.input_type)
        if dataset.synthetic:
            print("no idx files under data/%s: training on the deterministic synthetic stand-in" % dataset.datagroup)
    if model_name == "":
        model_name = model_str
    n_clusters = argv.n_clusters
    if n_clusters < 1:
        n_clusters = dataset.n_classes
    if argv.batch_size % world:
        raise ValueError("--batch_size must be divisible by the number of ranks")

    sess = Session()
    if model_str == "vade":           # train.py:199-203; its layer widths are literals of the class (2000,500,500 / 500,500,2000)
        model = base_models.VaDE(
            model_name, dataset.input_type, dataset.input_dim, argv.latent_dim, n_clusters,
            activation="relu", initializer="xavier", cnn=argv.cnn,
            batch_size=argv.batch_size // world, dtype=argv.dtype,
            noise="host" if argv.host_noise else "device", seed=argv.seed, session=sess, gmm=argv.gmm, eval=argv.eval, gmm_seeding=argv.gmm_seeding
        ).build_graph()
    else:
        model = base_models.DeepMixtureVAE(
            model_name, dataset.input_type, dataset.input_dim, argv.latent_dim, n_clusters,
            activation="relu", initializer="xavier", cnn=argv.cnn,
            batch_size=argv.batch_size // world, dtype=argv.dtype,
            enc_layers=[int(v) for v in argv.enc_layers.split(",")], head_dim=argv.head_dim,
            dec_layers=[int(v) for v in argv.dec_layers.split(",")], gumbel=argv.gumbel, temperature=argv.temperature,
            noise="host" if argv.host_noise else "device", seed=argv.seed, session=sess, gmm=argv.gmm, eval=argv.eval, gmm_seeding=argv.gmm_seeding,
            label_weight=argv.label_weight if argv.n_labeled > 0 else None
        ).build_graph()

    # dmvae trains on train + test rows (train.py:205-213)
    train_data = np.concatenate([dataset.train_data, dataset.test_data], axis=0)
    train_classes = np.concatenate([dataset.train_classes, dataset.test_classes], axis=0)
    # --binarize: the train set takes the named mode; a set that is evaluated only keeps ONE draw under "dynamic" (the protocol of Burda et al.)
    held_out = dict(binarize="static" if argv.binarize == "dynamic" else argv.binarize, binarize_seed=argv.binarize_seed)
    test_data = Dataset((dataset.test_data, dataset.test_classes), batch_size=argv.batch_size, **held_out)
    # --n_labeled: drawn from the train split's rows only (the first len(train split) rows of train_data): the test rows train unlabelled
    labeled = None
    if argv.n_labeled > 0:
        from includes.utils import choose_labeled
        labeled = choose_labeled(train_classes, argv.n_labeled, n_clusters, argv.label_seed, rows=np.arange(len(dataset.train_data)))
    train_data = Dataset((train_data, train_classes), batch_size=argv.batch_size, binarize=argv.binarize, binarize_seed=argv.binarize_seed,
                         labeled=labeled, augment=argv.augment, augment_seed=argv.augment_seed)

    # --knn votes among the train split alone (train_data holds the test rows too: each would find itself) and --probe fits on it;
    # unshuffled, so that nothing is drawn from the NumPy stream and the run trains as it does without the flags
    split_data = (Dataset((dataset.train_data, dataset.train_classes), batch_size=argv.batch_size, shuffle=False, **held_out)
                  if (argv.knn > 0 or argv.probe or argv.few_label > 0) and rank == 0 else None)
    if argv.binarize != "off":          # make the first draw now: the host views (plots, --pretrain's mixture fit) read it back from the device
        for ds in (test_data, train_data, split_data):
            if ds is not None:
                ds.device_rows(sess.device)
    knn_data = split_data if argv.knn > 0 else None
    probe_data = split_data if argv.probe else None
    few_data = split_data if argv.few_label > 0 else None

    model.define_train_step(argv.init_lr, train_data.epoch_len * argv.decay_epochs, argv.decay_rate)

    model.path = "saved-models/%s/%s" % (dataset.datagroup, model.name)
    if rank == 0:
        for path in [model.path + "/" + x for x in ["model", "vae", "prior"]]:
            if not os.path.exists(path):
                os.makedirs(path)
    if argv.pretrain:     # train.py:222-231, :241-249
        model.define_pretrain_step(argv.pretrain_vae_lr, argv.pretrain_prior_lr)
        model.pretrain(sess, train_data, argv.pretrain_epochs_vae, argv.pretrain_epochs_prior)
    ckpt_path = model.path + "/model/parameters.ckpt"
    try:      # the checkpoint is an npz archive of the trainables (as the pretraining stages write): no pickle
        with np.load(ckpt_path, allow_pickle=False) as f:
            model.load_state_dict({k: f[k] for k in f.files})
        if rank == 0:
            print("Restored", ckpt_path)
    except (OSError, ValueError, KeyError, RuntimeError, EOFError, zipfile.BadZipFile) as e:
        # no checkpoint, one written by another revision (e.g. a torch.save zip at this path), a truncated archive,
        # other shapes / names: say why and carry on from the initial parameters, as the reference does
        # (bare except around saver.restore, train.py:251-258) and as DeepMixtureVAE._restore does
        if rank == 0:
            print("Could not load trained model" + ("" if isinstance(e, FileNotFoundError) else " (%s: %s)" % (type(e).__name__, e)))
    if world > 1:   # every rank starts from rank 0's parameters
        import torch.distributed as dist
        dist.broadcast(model.engine.param, src=0)
        model.engine.refresh_shadow()

    from tqdm import tqdm
    maxAcc = 0.0
    with tqdm(range(argv.n_epochs), postfix={"loss": "inf", "accTrain": "0.00%", "accTest": "0.00%"}, disable=rank != 0) as bar:
        anneal_term = 0.0 if argv.kl_annealing else 1.0
        for epoch in bar:
            if epoch % argv.save_epochs == 0 and argv.debug:
                model.debug(sess, train_data)
            lmTest = None
            if plotting and epoch % argv.plot_epochs == 0:      # train.py:281-286
                visualization.mnist_sample_plot(model, sess, tsne=argv.tsne != "off", tsne_backend=argv.tsne if argv.tsne != "off" else "host")
                visualization.mnist_regeneration_plot(model, test_data, sess)
                if argv.latent_map != "off":
                    lmTest = visualization.latent_map_plot(model, test_data, sess, method=argv.latent_map, counter=epoch)
            if argv.kl_annealing and (epoch + 1) % argv.anneal_epochs == 0:
                anneal_term = min(anneal_term + argv.anneal_step, 1.0)
            loss = model.train_op(sess, train_data, anneal_term)
            t_eval = time.perf_counter()           # (train_op has synchronised; both get_accuracy modes end in a synchronising read-back)
            accTrain = model.get_accuracy(sess, train_data)
            accTest = model.get_accuracy(sess, test_data)
            eval_seconds = time.perf_counter() - t_eval
            accDirect = model.get_direct_accuracy(sess, test_data) if argv.n_labeled > 0 else None      # (no reshuffle: the NumPy stream stays put)
            llTest =model.get_log_likelihood(sess, test_data, k=argv.loglik, counter=epoch) if argv.loglik > 0 else None
            cmTest = model.get_cluster_metrics(sess, test_data, counter=epoch) if argv.metrics else None
            # (rank 0 alone: the call holds no collective and every rank would compute the same figures)
            pdTest = model.get_posterior_diagnostics(sess, test_data, counter=epoch) if argv.diagnostics and rank == 0 else None
            knnTest = model.get_knn_accuracy(sess, knn_data, test_data, k=argv.knn) if knn_data is not None else None
            probeTest = model.get_linear_probe_accuracy(sess, probe_data, test_data, C=argv.probe_C) if probe_data is not None else None
            flTest = (model.get_few_label_accuracy(sess, few_data, test_data, n_labeled=argv.few_label, seed=argv.few_label_seed)
                      if few_data is not None else None)
            acTest = (model.get_augmentation_consistency(sess, test_data, argv.aug_consistency, n_draws=argv.aug_draws, counter=epoch)
                      if argv.aug_consistency and rank == 0 else None)
            sqTest = model.get_sample_quality(sess, test_data, k=argv.sample_quality, counter=epoch) if argv.sample_quality > 0 and rank == 0 else None
            skTest = model.get_sample_distance(sess, test_data, counter=epoch) if argv.sample_distance and rank == 0 else None
            rqTest = model.get_reconstruction_quality(sess, test_data) if argv.recon_quality and rank == 0 else None
            sdTest = model.get_sample_diversity(sess, n_per_cluster=argv.sample_diversity, counter=epoch) if argv.sample_diversity > 0 and rank == 0 else None
            improved = accTest > maxAcc
            if world > 1:
                # the branch below holds a COLLECTIVE (sync_master): rank 0 decides and every rank follows.  Each rank scores the same
                # test set with the same weights, but an accuracy may still differ by a sample between ranks (VaDE's k noise draws from
                # the process-global NumPy RNG; a last-bit difference in a logit) -- ranks deciding for themselves could then split
                # at the all-gather and hang the job
                import torch
                import torch.distributed as dist
                flag = torch.tensor([1 if improved else 0], dtype=torch.int32, device=model.engine.device if dist.get_backend() == "nccl" else "cpu")
                dist.broadcast(flag, src=0)
                improved = bool(int(flag.item()))
            if improved:
                maxAcc = max(maxAcc, accTest)
                if world > 1:      # sharded bf16 steps leave a rank's fp32 weights current on its own slice only
                    from dmvae_hip import make_exchange
                    model.engine.sync_master(make_exchange(4 * model.engine.param.numel()))
                if rank == 0:
                    with open(ckpt_path + ".tmp", "wb") as f:
                        np.savez(f, **model.state_dict())
                    os.replace(ckpt_path + ".tmp", ckpt_path)
            if rank == 0:      # one JSON line per epoch (the reference has no metrics log; its tqdm postfix is the only record)
                ep = dict(getattr(model, "last_epoch", None) or {})
                sec = ep.pop("seconds", None)
                rec = dict(epoch=epoch, **ep, images_per_sec=(ep.get("rows", 0) / sec if sec else None), train_seconds=sec,
                           acc_train=float(accTrain), acc_test=float(accTest), max_acc=float(max(maxAcc, accTest) if improved else maxAcc),
                           eval_seconds=eval_seconds, eval=argv.eval, world=world, batch_size=argv.batch_size, dtype=argv.dtype, model=model_str,
                           binarize=argv.binarize, augment=str(train_data.augment) if train_data.augment is not None else "off")
                if accDirect is not None:      # (label_xent / label_rows / label_acc are in last_epoch)
                    rec.update(acc_direct_test=float(accDirect), n_labeled=argv.n_labeled, label_weight=argv.label_weight)
                if llTest is not None:
                    rec.update(ll_test=float(llTest), loglik_draws=argv.loglik)
                if cmTest is not None:
                    rec.update(_metrics_record(cmTest))
                if pdTest is not None:
                    rec.update(_diagnostics_record(pdTest))
                if knnTest is not None:
                    rec.update(knnTest=float(knnTest), knn_k=argv.knn)
                if probeTest is not None:
                    rec.update(probeTest=float(probeTest), probe_C=argv.probe_C, probe_iters=model.last_linear_probe_.n_iter_)
                if flTest is not None:
                    rec.update(_few_label_record(flTest))
                if acTest is not None:
                    rec.update(aug_agree=float(acTest["agree"]), aug_acc=float(acTest["acc_aug"]), aug_acc_clean=float(acTest["acc_clean"]),
                               aug_agree_per_class=[None if math.isnan(x) else float(x) for x in acTest["agree_per_class"]])
                if sqTest is not None:
                    rec.update(_sample_quality_record(sqTest))
                if skTest is not None:
                    rec.update(_sample_distance_record(skTest))
                rec.update(_ssim_record(rqTest, sdTest))
                if lmTest is not None:
                    rec.update(lmTrust=float(lmTest["trustworthiness"]), lmKL=float(lmTest["kl"]), lm_method=lmTest["method"],
                               lm_seconds=float(lmTest["seconds"]))
                with open(argv.model + "_metrics.jsonl", "a") as fl:
                    fl.write(json.dumps(rec) + "\n")
            if math.isnan(loss):
                raise FloatingPointError("loss is NaN at epoch %d (the reference drops into pdb here, train.py:320-321)" % epoch)
            postfix = {"loss": "%.4f" % loss, "accTrain": "%.4f" % accTrain, "accTest": "%.4f" % accTest,
                       "maxAcc": "%.4f" % maxAcc, "accClusteringTest": "%.4f" % accTest}
            if accDirect is not None:
                postfix["accDirect"] = "%.4f" % accDirect
            if llTest is not None:
                postfix["llTest"] = "%.4f" % llTest
            if cmTest is not None:
                postfix.update(nmiTest="%.4f" % cmTest["nmi"], silTest="%.4f" % cmTest["silhouette"])
            if pdTest is not None:
                postfix.update(miTest="%.4f" % pdTest["mi"], auTest="%d" % pdTest["active_units"])
            if knnTest is not None:
                postfix["knnTest"] = "%.4f" % knnTest
            if probeTest is not None:
                postfix["probeTest"] = "%.4f" % probeTest
            if flTest is not None:
                postfix["flTest"] = "%.4f" % flTest["accuracy"]
            if acTest is not None:
                postfix["augAgree"] = "%.4f" % acTest["agree"]
            if sqTest is not None:
                postfix.update(precTest="%.4f" % sqTest["precision"], covTest="%.4f" % sqTest["coverage"])
            if skTest is not None:
                postfix["sdTest"] = "%.4f" % skTest["divergence"]
            if rqTest is not None:
                postfix.update(ssimTest="%.4f" % rqTest["ssim"], psnrTest="%.2f" % rqTest["psnr"])
            if sdTest is not None:
                postfix["divTest"] = "%.4f" % float(np.mean(sdTest["ssim_within"]))
            bar.set_postfix(postfix)
    if plotting:                                                  # train.py:332-334
        visualization.mnist_sample_plot(model, sess, tsne=argv.tsne != "off", tsne_backend=argv.tsne if argv.tsne != "off" else "host")
        visualization.mnist_regeneration_plot(model, test_data, sess)
        if argv.latent_map != "off":                              # the whole train set: above 32768 rows "auto" takes the knn form
            visualization.latent_map_plot(model, train_data, sess, method=argv.latent_map, counter=argv.n_epochs)
    if rank == 0:
        with open(argv.model + "_logs.txt", "a+") as fl:
            fl.write("\n" + str(argv) + "\n------\n")
            fl.write("Max Accuracy        " + str(maxAcc) + "\n============")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return loss


def main_moe(argv, world, rank):
    """train.py:146-180, 241-245, 295-297 of the reference: the mixture-of-experts models on separate train / test sets"""
    import models
    from dmvae_hip import Session
    from includes.utils import MEDataset
    if argv.augment or argv.aug_consistency:
        raise ValueError("--augment / --aug_consistency with --model %s: the regression labels are functions of the grey rows; the MoE data set is not "
                         "augmented" % argv.model)
    if argv.binarize != "off":
        raise ValueError("--binarize %s with --model %s: the regression labels are functions of the grey rows; the MoE data set is not binarised"
                         % (argv.binarize, argv.model))
    if world > 1:
        raise NotImplementedError("--model %s: MoE models train on one rank" % argv.model)
    if argv.pretrain:
        raise NotImplementedError("--pretrain with a MoE model is not built")
    if argv.cnn:
        raise NotImplementedError("--cnn with a MoE model: the flat input the experts read is not resident in conv plans")
    from includes.utils import load_data
    dataset = load_data(argv.dataset, classification=argv.classification, output_dim=argv.output_dim, moe=True)
    output_dim = dataset.n_classes if argv.classification else argv.output_dim      # train.py:150-151
    sess = Session()
    kw = dict(activation="relu", initializer="xavier", featLearn=argv.featLearn, batch_size=argv.batch_size, dtype=argv.dtype,
              enc_layers=[int(v) for v in argv.enc_layers.split(",")], head_dim=argv.head_dim,
              dec_layers=[int(v) for v in argv.dec_layers.split(",")], gumbel=argv.gumbel, temperature=argv.temperature,
              noise="host" if argv.host_noise else "device", seed=argv.seed, session=sess, eval=argv.eval)
    name = argv.model_name or argv.model
    if argv.model == "dmoe":
        model = models.DeepMoE(name, dataset.input_type, dataset.input_dim, output_dim, argv.n_experts, argv.classification, **kw)
    else:
        model = models.DeepVariationalMoE(name, dataset.input_type, dataset.input_dim, argv.latent_dim, output_dim, argv.n_experts,
                                          argv.classification, **kw)
    model.build_graph()
    train_data = MEDataset((dataset.train_data, dataset.train_classes, dataset.train_labels), batch_size=argv.batch_size)
    test_data = MEDataset((dataset.test_data, dataset.test_classes, dataset.test_labels), batch_size=argv.batch_size)
    model.define_train_step(argv.init_lr, train_data.epoch_len * argv.decay_epochs, argv.decay_rate)
    model.path = "saved-models/%s/%s" % (dataset.datagroup, model.name)
    os.makedirs(model.path + "/model", exist_ok=True)
    ckpt_path = model.path + "/model/parameters.ckpt"
    try:
        with np.load(ckpt_path, allow_pickle=False) as f:
            model.load_state_dict({k: f[k] for k in f.files})
        print("Restored", ckpt_path)
    except (OSError, ValueError, KeyError, RuntimeError, EOFError, zipfile.BadZipFile) as e:
        print("Could not load trained model" + ("" if isinstance(e, FileNotFoundError) else " (%s: %s)" % (type(e).__name__, e)))
    maxAcc = -np.inf
    loss = float("nan")
    anneal_term = 0.0 if argv.kl_annealing else 1.0
    for epoch in range(argv.n_epochs):
        if argv.kl_annealing and (epoch + 1) % argv.anneal_epochs == 0:
            anneal_term = min(anneal_term + argv.anneal_step, 1.0)
        loss, batch_acc, loss_cls = model.train_op(sess, train_data, anneal_term)
        t_eval = time.perf_counter()
        accTrain, accClTrain = model.get_accuracy(sess, train_data)
        accTest, accClTest = model.get_accuracy(sess, test_data)
        eval_seconds = time.perf_counter() - t_eval
        cmTest = model.get_cluster_metrics(sess, test_data, counter=epoch) if argv.metrics else None
        knnTest = model.get_knn_accuracy(sess, train_data, test_data, k=argv.knn) if argv.knn > 0 else None
        probeTest = model.get_linear_probe_accuracy(sess, train_data, test_data, C=argv.probe_C) if argv.probe else None
        flTest = (model.get_few_label_accuracy(sess, train_data, test_data, n_labeled=argv.few_label, seed=argv.few_label_seed)
                  if argv.few_label > 0 else None)
        sqTest = model.get_sample_quality(sess, test_data, k=argv.sample_quality, counter=epoch) if argv.sample_quality > 0 else None
        skTest = model.get_sample_distance(sess, test_data, counter=epoch) if argv.sample_distance else None
        rqTest = model.get_reconstruction_quality(sess, test_data) if argv.recon_quality else None
        sdTest = model.get_sample_diversity(sess, n_per_cluster=argv.sample_diversity, counter=epoch) if argv.sample_diversity > 0 else None
        if accTest > maxAcc:
            maxAcc = accTest
            with open(ckpt_path + ".tmp", "wb") as f:
                np.savez(f, **model.state_dict())
            os.replace(ckpt_path + ".tmp", ckpt_path)
        rec = dict(epoch=epoch, loss=float(loss), loss_moe=float(loss_cls), batch_acc=float(batch_acc), acc_train=float(accTrain),
                   acc_test=float(accTest), acc_clustering_train=float(accClTrain), acc_clustering_test=float(accClTest),
                   max_acc=float(maxAcc), kl_ratio=float(anneal_term), eval_seconds=eval_seconds, eval=argv.eval, batch_size=argv.batch_size,
                   dtype=argv.dtype, model=argv.model)
        if cmTest is not None:
            rec.update(_metrics_record(cmTest))
        if knnTest is not None:
            rec.update(knnTest=float(knnTest), knn_k=argv.knn)
        if probeTest is not None:
            rec.update(probeTest=float(probeTest), probe_C=argv.probe_C, probe_iters=model.last_linear_probe_.n_iter_)
        if flTest is not None:
            rec.update(_few_label_record(flTest))
        if sqTest is not None:
            rec.update(_sample_quality_record(sqTest))
        if skTest is not None:
            rec.update(_sample_distance_record(skTest))
        rec.update(_ssim_record(rqTest, sdTest))
        with open(argv.model + "_metrics.jsonl", "a") as fl:
            fl.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
        if math.isnan(loss):
            raise FloatingPointError("loss is NaN at epoch %d" % epoch)
    return loss


if __name__ == "__main__":
    args = parser.parse_args()
    print(args)
    main(args)
