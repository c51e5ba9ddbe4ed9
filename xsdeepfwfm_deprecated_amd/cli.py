"""The reference harness around the model: utils/parameters.py (get_parser: the same flags and
defaults), utils/util.py (get_logger, get_model, load_model_dic).  `main_all.py` at the repo root is the
entry point that uses them."""
from __future__ import annotations

import argparse
import logging
import os
import sys

import torch

from .DeepFMs import DeepFMs


def parse_lr_schedule(spec):
    """"1:1e-4,2000:1e-3,200000:1e-4" -> [(1, 1e-4), (2000, 1e-3), (200000, 1e-4)]: the (step, lr) knots of
    FusedTrainStep(lr_schedule=...) under the rules of include/dfwfm_lr_schedule.h (1 to 64 knots, integer steps
    strictly increasing from >= 1, every lr finite and >= 0).  An argparse type: a malformed spec is a usage error."""
    import math
    knots = []
    for part in spec.split(","):
        try:
            step, lr = part.split(":")
            knots.append((int(step.strip()), float(lr)))
        except ValueError:
            raise argparse.ArgumentTypeError(f"lr schedule knot {part!r} is not STEP:LR") from None
    if not 1 <= len(knots) <= 64:
        raise argparse.ArgumentTypeError(f"an lr schedule has 1 to 64 knots, not {len(knots)}")
    for i, (step, lr) in enumerate(knots):
        if step < 1 or (i and step <= knots[i - 1][0]):
            raise argparse.ArgumentTypeError("lr schedule steps must be strictly increasing from >= 1")
        if not (math.isfinite(lr) and lr >= 0):
            raise argparse.ArgumentTypeError(f"lr schedule rate {lr!r} is not finite and >= 0")
    return knots


def get_parser():
    """utils/parameters.py:2-51 (flags, defaults and help as the reference) + -data_root."""
    p = argparse.ArgumentParser(description="Hyperparameter tuning and selection")
    a = p.add_argument
    a("-c", default="DeepFwFM", type=str, help="Models: FM, DeepFwFM ...")
    a("-use_cuda", default=1, type=int, help="Use CUDA or not")
    a("-gpu", default=0, type=int, help="GPU id")
    a("-n_epochs", default=8, type=int, help="Number of epochs")
    a("-numerical", default=13, type=int, help="Numerical features, 13 for Criteo")
    a("-use_multi", default="0", type=int, help="Use multiple CUDAs")
    a("-use_logit", default=0, type=int, help="Use Logistic regression")
    a("-use_fm", default=0, type=int, help="Use FM module or not")
    a("-use_fwlw", default=0, type=int, help="If to include FwFM linear weights or not")
    a("-use_lw", default=1, type=int, help="If to include FM linear weights or not")
    a("-use_ffm", default=0, type=int, help="Use FFM module or not")
    a("-use_fwfm", default=1, type=int, help="Use FwFM module or not")
    a("-use_deep", default=1, type=int, help="Use Deep module or not")
    a("-num_deeps", default=1, type=int, help="Number of deep networks")
    a("-deep_nodes", default=400, type=int, help="Nodes in each layer")
    a("-h_depth", default=3, type=int, help="Deep layers")
    a("-prune", default=0, type=int, help="Prune model or not")
    a("-prune_r", default=0, type=int, help="Prune r")
    a("-prune_deep", default=1, type=int, help="Prune Deep component")
    a("-prune_fm", default=1, type=int, help="Prune FM component")
    a("-emb_r", default=1., type=float, help="Sparse FM ratio over Sparse Deep ratio")
    a("-emb_corr", default=1., type=float, help="Sparse Corr ratio over Sparse Deep ratio")
    a("-sparse", default=0.9, type=float, help="Sparse rate")
    a("-warm", default=10, type=float, help="Warm up epochs before pruning")
    a("-ensemble", default=0, type=int, help="Ensemble models or not")
    a("-embedding_size", default=10, type=int, help="Embedding size")
    a("-batch_size", default=2048, type=int, help="Batch size")
    a("-random_seed", default=42, type=int, help="Random seed")
    a("-learning_rate", default=0.001, type=float, help="Learning rate")
    a("-momentum", default=0, type=float, help="Momentum")
    a("-l2", default=3e-7, type=float, help="L2 penalty")
    a("-dataset", default="criteo", type=str, help="Dataset to use",
      choices=["criteo", "tiny-criteo", "twitter", "ali", "avazu"])
    a("-save_model_path", default=0, type=str, help="Saved model path")
    a("-dynamic_quantization", default=0, type=int, help="Apply dynamic network quantization")
    a("-static_quantization", default=0, type=int, help="Apply static network quantization")
    a("-quantization_aware", default=0, type=int, help="Quantization Aware Training")
    a("-kd", default=0, type=int, help="Perform knowledge distillation")
    a("-loss_type", default="logloss", type=str, help="Used loss (should be logloss but for kd we need softmax)")
    # the README's spellings (-embedding_bag / -qr_flag, reference README.md:107,117) are rejected by the
    # reference parser (probe P5); both spellings are accepted here, same destination
    a("-emb_bag", "-embedding_bag", dest="emb_bag", default=0, type=int, help="Use embedding bag")
    a("-qr_emb", "-qr_flag", dest="qr_emb", default=0, type=int, help="Use QR Embeddings")
    a("-qr_operation", default="mult", type=str)
    a("-qr_collisions", default=4, type=int)
    a("-qr_threshold", default=200, type=int)
    a("-twitter_category", default="like", type=str, choices=["reply", "retweet", "retweet_comment", "like"])
    a("-time_on_cuda", default=0, type=int)
    a("-data_root", default=".", type=str, help="directory holding data/ (this engine's addition)")
    a("-mlp_dtype", default="f32", type=str, choices=["f32", "bf16", "int8"],
      help="deep tower of the inference forward: f32, bf16 MFMA with f32 accumulation, or int8 MFMA with per-neuron "
           "weight and per-row activation scales (HIP only; this engine's addition, DeepFMs.mlp_dtype)")
    a("-bf16_fused", default=0, type=int, choices=[0, 1],
      help="with -mlp_dtype bf16: the bf16 forward as one launch, and batch sets of it in the evaluation "
           "(DeepFMs.bf16_fused; the same logits; an unsupported shape keeps the per-layer path)")
    a("-bf16_fold", default=0, type=int, choices=[0, 1],
      help="with -mlp_dtype bf16 -bf16_fused 1: the numerical fields folded into layer 1 of the one-launch bf16 "
           "forward (DeepFMs.bf16_fold; another rounding of the same size; a model that cannot fold stays unfolded)")
    a("-table_dtype", default="f32", type=str, choices=["f32", "fp16", "int8"],
      help="storage of the inference forward's serving copy of the categorical tables: f32, or fp16 second-order rows "
           "rounded once per weight update, half the bytes, or int8 second-order rows under one bf16 scale per row, a "
           "quarter of the bytes (HIP only; this engine's addition, DeepFMs.table_dtype; "
           "QR tables, the small-batch, per-layer bf16 and sparse paths raise)")
    a("-lazy_adam", default=0, type=int, choices=[0, 1],
      help="training on a HIP device with Adam: the categorical tables' Adam updates only the rows each batch touched "
           "(DeepFMs.lazy_table_adam; SparseAdam / LazyAdam semantics, NOT the reference's dense Adam: untouched rows "
           "get no moment decay and no L2)")
    a("-lr_schedule", default=None, type=parse_lr_schedule, metavar="STEP:LR[,STEP:LR...]",
      help="training on a HIP device with Adam: a piecewise-linear learning-rate schedule evaluated on the device "
           "inside the graph-replayed step, e.g. \"1:1e-4,2000:1e-3,200000:1e-4\" for a warm-up and a decay "
           "(DeepFMs.lr_schedule; steps count Adam steps from 1, constant before the first and after the last knot; "
           "-learning_rate is then unused)")
    a("-fused_optimizer", default=0, type=int, choices=[0, 1],
      help="training on a HIP device: optimizer_type 'sgd', 'adag' and 'rmsp' run on the graph-replayed fused step too "
           "(DeepFMs.fused_optimizer, include/dfwfm_optim.h) instead of autograd + torch.optim; fit() raises when the "
           "fused step is not the path")
    a("-lazy_tables", default=0, type=int, choices=[0, 1],
      help="training on a HIP device on the fused step: the categorical tables' update touches only the rows each "
           "batch touched, whichever optimizer runs (DeepFMs.lazy_tables, include/dfwfm_lazy_optim.h; with Adam the "
           "same as -lazy_adam).  Plain SGD and Adagrad without -l2 give the dense step's exact bits; momentum-SGD, "
           "RMSprop and any -l2 are NOT the dense optimizer: untouched rows get no decay and no L2")
    a("-lazy_exchange", default=0, type=int, choices=[0, 1],
      help="data-parallel training with -lazy_adam / -lazy_tables: the touched rows are those of the GLOBAL batch, "
           "the union of the ranks' exchanged touched-row lists (DeepFMs.lazy_exchange, include/dfwfm_lazy_lists.h); "
           "without it the lazy switches are refused under torch.distributed")
    a("-rowwise_adagrad", default=0, type=int, choices=[0, 1],
      help="training on a HIP device with optimizer_type 'adag' and -fused_optimizer 1: the categorical tables are "
           "trained with row-wise Adagrad, one accumulator per table row fed with the mean of the row's squared "
           "gradient, over the rows each batch touched (DeepFMs.rowwise_adagrad, include/dfwfm_rowwise_adagrad.h); "
           "NOT the reference's element-wise Adagrad; one process only, unless -rowwise_exchange 1")
    a("-rowwise_exchange", default=0, type=int, choices=[0, 1],
      help="data-parallel training with -rowwise_adagrad: the rows of the GLOBAL batch, the union of the ranks' "
           "exchanged touched-row lists, get the row-wise update on every replica (DeepFMs.rowwise_exchange, "
           "include_dp/dfwfm_rowwise_lists.h); without it -rowwise_adagrad is refused under torch.distributed")
    return p


def get_logger(filename=None, log_dir="./logs"):
    """utils/util.py:22-40 (stdout + ./logs/<name>.log)."""
    root = logging.getLogger("xsDeepFwFM")
    root.setLevel(logging.DEBUG)
    fmt = logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    h = logging.StreamHandler(sys.stdout)
    h.setLevel(logging.DEBUG)
    h.setFormatter(fmt)
    root.addHandler(h)
    if filename:
        os.makedirs(log_dir, exist_ok=True)
        # string concatenation as the reference ('./logs/' + filename): main_all's name starts with '/'
        fh = logging.FileHandler(filename=log_dir + "/" + filename + ".log")
        fh.setLevel(logging.DEBUG)
        fh.setFormatter(fmt)
        root.addHandler(fh)
    root.propagate = False
    return root


def load_model_dic(model, model_file, sparse=False):
    """utils/util.py:43-53; files this engine wrote are plain state dicts (weights_only load)."""
    state_dict = torch.load(model_file, weights_only=True, map_location="cpu")
    if sparse:
        model.load_state_dict(state_dict, strict=False)  # the reference's to_sparse() result is discarded
    else:
        model.load_state_dict(state_dict)
    return model


def get_model(cuda, feature_sizes, pars, dynamic_quantization=False, static_quantization=False,
              quantization_aware=False, field_size=39, deep_nodes=400, h_depth=3, logger=None):
    """utils/util.py:56-73."""
    m = DeepFMs(field_size=field_size, feature_sizes=feature_sizes, embedding_size=pars.embedding_size,
                n_epochs=pars.n_epochs, verbose=False, use_cuda=cuda, use_fm=pars.use_fm, use_fwfm=pars.use_fwfm,
                use_ffm=pars.use_ffm, use_deep=pars.use_deep, batch_size=pars.batch_size,
                learning_rate=pars.learning_rate, weight_decay=pars.l2, momentum=pars.momentum,
                sparse=pars.sparse, warm=pars.warm, h_depth=pars.h_depth, deep_nodes=pars.deep_nodes,
                num_deeps=pars.num_deeps, numerical=pars.numerical, use_lw=pars.use_lw, use_fwlw=pars.use_fwlw,
                use_logit=pars.use_logit, random_seed=pars.random_seed, quantization_aware=quantization_aware,
                dynamic_quantization=dynamic_quantization, static_quantization=static_quantization,
                loss_type=pars.loss_type, embedding_bag=pars.emb_bag, qr_flag=pars.qr_emb,
                qr_operation=pars.qr_operation, qr_collisions=pars.qr_collisions, qr_threshold=pars.qr_threshold,
                logger=logger)
    m.mlp_dtype = getattr(pars, "mlp_dtype", "f32")  # a CPU model with "bf16" raises at its first forward
    m.bf16_fused = bool(getattr(pars, "bf16_fused", 0))
    m.bf16_fold = bool(getattr(pars, "bf16_fold", 0))
    m.table_dtype = getattr(pars, "table_dtype", "f32")  # a CPU model with "fp16" or "int8" raises at its first forward
    m.lazy_table_adam = bool(getattr(pars, "lazy_adam", 0))  # fit() raises if the fused Adam step is not the path
    m.lr_schedule = getattr(pars, "lr_schedule", None)  # fit() raises if the fused Adam step is not the path
    m.fused_optimizer = bool(getattr(pars, "fused_optimizer", 0))  # fit() raises if the fused step is not the path
    m.lazy_tables = bool(getattr(pars, "lazy_tables", 0))  # fit() raises if the fused step is not the path
    m.lazy_exchange = bool(getattr(pars, "lazy_exchange", 0))  # fit() raises without ranks or a lazy switch
    m.rowwise_adagrad = bool(getattr(pars, "rowwise_adagrad", 0))  # fit() raises off the fused Adagrad step
    m.rowwise_exchange = bool(getattr(pars, "rowwise_exchange", 0))  # fit() raises without ranks or rowwise_adagrad
    return m
