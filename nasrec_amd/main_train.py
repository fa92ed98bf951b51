"""Train and evaluate one model — the engine-side counterpart of the reference's nasrec/main_train.py with the same flags,
defaults, printouts, log pickle and checkpoint, so the published recipes (scripts/eval_best_model/*.sh) run verbatim:

    python -u nasrec_amd/main_train.py --root_dir ./data/criteo_kaggle_autoctr/ --net supernet-config \\
        --supernet_config nasrec_amd/configs/criteo/ea_criteo_kaggle_xlarge_best_1shot.json --num_epochs 1 \\
        --learning_rate 0.16 --train_batch_size 256 --wd 0 --logging_dir ./experiments/... --gpu 0 --test_interval 10000

Differences: `--root_dir synthetic[:steps=N,...]` generates dataset-shaped random batches (the datasets cannot be shipped);
the TensorBoard graph dump (a jit trace of the model, main_train.py:129-137) is skipped — the network is one launch plan,
not a traceable module graph — and the scalar writer is used only if tensorboard is installed."""
import argparse
import json
import os
import sys
import warnings

sys.path.append(os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from nasrec_amd.supernet.modules import flags  # noqa: E402
from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib  # noqa: E402
from nasrec_amd.utils.config import NUM_EMBEDDINGS_AVAZU, NUM_EMBEDDINGS_CRITEO, NUM_EMBEDDINGS_KDD  # noqa: E402
from nasrec_amd.utils.data_pipes import make_loaders  # noqa: E402
from nasrec_amd.utils.io_utils import create_dir, dump_pickle_data, load_json, save_model_checkpoint  # noqa: E402
from nasrec_amd.utils.lr_schedule import ConstantWithWarmup, CosineAnnealingWarmupRestarts  # noqa: E402
from nasrec_amd.utils.train_utils import (L2Loss, get_model_flops_and_params, init_weights, train_and_test_one_epoch,  # noqa: E402
                                          warmup_model)

warnings.simplefilter("ignore", ResourceWarning)
warnings.simplefilter("ignore", UserWarning)

_num_sparse_inputs_dict = {"criteo-kaggle": 26, "avazu": 23, "kdd": 10}
_num_embedding_dict = {"criteo-kaggle": NUM_EMBEDDINGS_CRITEO, "avazu": NUM_EMBEDDINGS_AVAZU, "kdd": NUM_EMBEDDINGS_KDD}


def summary_writer(logging_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(logging_dir)
    except Exception:  # tensorboard not installed
        return None


TABLE_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def check_table_dtype(args, world: int = 1, use_amp: bool = False, last_layer: bool = False):
    """--table-dtype bf16 at start-up: the recipe must be the one the fused step has for bf16 tables (--optimizer adam-adagrad-tables
    --table-rowwise, one process, whole tables, nothing else that reads or writes a table row) — anything else is a ValueError that
    names the flag, never a silent torch route (which could not train them: utils/optim.AdamAdagradTables.step raises).
    world / use_amp / last_layer: what the caller knows beyond the flags (the process group's size, torch.autocast, the last-layer
    fine-tune mode)"""
    if getattr(args, "table_dtype", "fp32") != "bf16":
        return
    head = "--table-dtype bf16 "
    if args.optimizer != "adam-adagrad-tables" or not getattr(args, "table_rowwise", False):
        raise ValueError(head + "needs --optimizer adam-adagrad-tables --table-rowwise (got --optimizer %s%s): row-wise Adagrad in fp32 on "
                         "the widened row, stored with stochastic rounding, is the one rule bf16 tables train with"
                         % (args.optimizer, " --table-rowwise" if getattr(args, "table_rowwise", False) else ""))
    if getattr(args, "ema", 0.0):
        raise ValueError(head + "with --ema: the weight average keeps fp32 shadow tables; not built for bf16 tables")
    if getattr(args, "decoupled_wd", 0.0):
        raise ValueError(head + "with --decoupled-wd: the lazily paid decay rewrites fp32 table rows; not built for bf16 tables")
    if args.wd:
        from nasrec_amd.optim_spec import regularises_tables
        if regularises_tables(args.wd, args.no_reg_param_name):
            raise ValueError(head + "with --wd %r reaching the embedding tables: every row would move every step (--wd 0, the published "
                             "recipes' value)" % (args.wd,))
        raise ValueError(head + "with --wd %r: weight decay's launches are not built for bf16 tables (--wd 0)" % (args.wd,))
    if use_amp:
        raise ValueError(head + "with AMP (use_amp): autocast keeps the torch route, which cannot train bf16 tables")
    if getattr(args, "table_sharding", "none") == "row":
        raise ValueError(head + "with --table-sharding row: bf16 tables are whole tables on one device")
    if world > 1:
        raise ValueError(head + "with a world size of %d: the data-parallel step is not built for bf16 tables (one process)" % world)
    if last_layer:
        raise ValueError(head + "with the last-layer fine-tune mode: its fused step and its torch route both take fp32 tables")


def _cowclip(text):
    from nasrec_amd.utils.optim import parse_cowclip
    try:
        return parse_cowclip(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_cowclip_flag(p):
    p.add_argument("--cowclip", type=_cowclip, default=None, metavar="R[,ZETA]",
                   help="CowClip (Zheng et al., AAAI 2023), absent = off: behind the global clip every embedding row the batch touches has "
                        "its summed gradient held to cnt * max(R * |w|, ZETA), cnt = how often its id occurs in the batch (ZETA defaults "
                        "to 1e-5; utils/optim.CowClip) - what a large --train_batch_size needs.  Inside the fused step under every "
                        "--optimizer, by CowClip.apply() on the torch route; one process, whole fp32 tables, no --wd on the tables")


def check_cowclip(args, world: int = 1, last_layer: bool = False):
    """--cowclip at start-up, from the flags alone: what CowClip is not built for is a ValueError that names the flag
    (train_utils.refuse_cowclip asks the model and the optimizer the same questions before the first step)"""
    if getattr(args, "cowclip", None) is None:
        return
    head = "--cowclip "
    if getattr(args, "table_dtype", "fp32") == "bf16":
        raise ValueError(head + "with --table-dtype bf16: CowClip reads fp32 table rows; not built for bf16 tables")
    if args.wd:
        from nasrec_amd.optim_spec import regularises_tables
        if regularises_tables(args.wd, args.no_reg_param_name):
            raise ValueError(head + "with --wd %r reaching the embedding tables: the L2 term's 2 wd W would be clipped with the gradient "
                             "(--no-reg-param-name _embedding leaves the tables out, or --wd 0)" % (args.wd,))
    if getattr(args, "table_sharding", "none") == "row":
        raise ValueError(head + "with --table-sharding row: a row-sharded table holds one rank's rows; CowClip needs whole tables")
    if world > 1:
        raise ValueError(head + "with a world size of %d: the ids' counts would have to be global; one process" % world)
    if last_layer:
        raise ValueError(head + "with the last-layer fine-tune mode: the tables are frozen there, nothing to clip")


def build_cowclip(args, model):
    """the CowClip helper of a run with --cowclip (over the model's tables), or None"""
    if getattr(args, "cowclip", None) is None:
        return None
    from nasrec_amd.utils.optim import CowClip
    return CowClip(list(model._embedding.parameters()), *args.cowclip)


def add_table_dtype_flags(p):
    p.add_argument("--table-dtype", dest="table_dtype", type=str, default="fp32", choices=sorted(TABLE_DTYPES),
                   help="storage type of the embedding tables (SuperNet(table_dtype=...)): bf16 halves their memory and their checkpoint; "
                        "needs --optimizer adam-adagrad-tables --table-rowwise, one process, --wd 0 and neither --ema nor --decoupled-wd")
    p.add_argument("--table-seed", dest="table_seed", type=int, default=0,
                   help="--table-dtype bf16: seed of the stochastic rounding the tables' new weights are stored with")


def build_optimizer(name, model, lr, table_lr_scale=1.0, table_eps=1e-2, table_rowwise=False, table_seed=0):
    """main_train.py:150-160 (Adagrad eps 1e-2; Adam eps 1e-8; SGD nesterov momentum 0.9); row-sparse-adam: Adam's lr and eps, the
    tables moving in the batch's rows only (utils/optim.RowSparseAdam); rowwise-adam: the same with one second-moment float per
    table row (utils/optim.RowwiseSparseAdam); rmsprop: torch's defaults (alpha 0.99, eps 1e-8) as
    utils/optim.LazyRMSprop, which is torch.optim.RMSprop and the type the fused step takes; adam-adagrad-tables: Adam's lr and eps
    on the dense parameters, Adagrad with lr * table_lr_scale and table_eps on the tables (utils/optim.AdamAdagradTables), row-wise
    Adagrad with table_rowwise — which goes with that optimizer only; table_seed: the stochastic rounding's seed of bf16 tables"""
    if table_rowwise and name != "adam-adagrad-tables":
        raise ValueError("--table-rowwise is the tables' rule of --optimizer adam-adagrad-tables; it does nothing with --optimizer %s" % name)
    if name == "adagrad":
        return torch.optim.Adagrad(model.parameters(), lr=lr, eps=1e-2)
    if name == "adam":
        return torch.optim.Adam(model.parameters(), lr=lr, eps=1e-8)
    if name == "sgd":
        return torch.optim.SGD(model.parameters(), lr=lr, nesterov=True, momentum=0.9)
    if name == "row-sparse-adam":
        from nasrec_amd.utils.optim import RowSparseAdam
        if getattr(model, "_table_sharding", None) == "row":
            raise ValueError("--optimizer row-sparse-adam needs whole tables: a row-sharded table holds one rank's rows under local ids; "
                             "use --optimizer adam with --table-sharding row")
        return RowSparseAdam(model.parameters(), list(model._embedding.parameters()), lr=lr, eps=1e-8)
    if name == "rowwise-adam":
        from nasrec_amd.utils.optim import RowwiseSparseAdam
        if getattr(model, "_table_sharding", None) == "row":
            raise ValueError("--optimizer rowwise-adam needs whole tables: a row-sharded table holds one rank's rows under local ids; "
                             "use --optimizer adam with --table-sharding row")
        return RowwiseSparseAdam(model.parameters(), list(model._embedding.parameters()), lr=lr, eps=1e-8)
    if name == "adam-adagrad-tables":
        from nasrec_amd.utils.optim import AdamAdagradTables
        return AdamAdagradTables(model.parameters(), list(model._embedding.parameters()), lr=lr, eps=1e-8, table_lr_scale=table_lr_scale,
                                 table_eps=table_eps, table_rowwise=table_rowwise, table_seed=table_seed)
    if name == "rmsprop":
        from nasrec_amd.utils.optim import LazyRMSprop
        return LazyRMSprop(model.parameters(), lr=lr)
    raise KeyError(name)


def build_lr_scheduler(kind, optimizer, num_train_steps, num_warmup_steps, max_lr):
    if kind == "cosine":
        return CosineAnnealingWarmupRestarts(optimizer, first_cycle_steps=num_train_steps, warmup_steps=num_warmup_steps, max_lr=max_lr,
                                             min_lr=1e-8)
    if kind == "constant":
        return ConstantWithWarmup(optimizer, num_warmup_steps=num_warmup_steps)
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[num_train_steps * 10], gamma=0.1)  # "constant-no-warmup"


def train_and_eval_one_model(model, args):
    train_loader, test_loader = make_loaders(args)
    with torch.no_grad():
        model = warmup_model(model, train_loader, args.gpu)
    flops, params = get_model_flops_and_params(model, train_loader, args.gpu)
    print("FLOPS: {:.4f} M \t Params: {:.4f} M".format(flops / 1e6, params / 1e6))
    if args.loss_function != "bce":
        raise NotImplementedError("Loss function {} is not implemented!".format(args.loss_function))
    loss_fn = torch.nn.BCEWithLogitsLoss()
    writer = summary_writer(args.logging_dir)
    flags.config_debug(False)

    l2_loss_fn = L2Loss(args.wd, args.no_reg_param_name, gpu=args.gpu)  # (a spec the fused engine step folds in: any --wd)

    optimizer = build_optimizer(args.optimizer, model, args.learning_rate, args.table_lr_scale, args.table_eps,
                                table_rowwise=args.table_rowwise, table_seed=args.table_seed)
    steps_per_epoch = args.train_limit // args.train_batch_size
    num_train_steps = steps_per_epoch * args.num_epochs
    num_warmup_steps = steps_per_epoch // 10 // args.num_epochs
    lr_scheduler = build_lr_scheduler(args.lr_schedule, optimizer, num_train_steps, num_warmup_steps, args.learning_rate)
    model.apply(init_weights)
    from nasrec_amd.utils.dist import assert_replicas_identical, broadcast_replica_state
    broadcast_replica_state(model)  # data parallel: rank 0's weights, tables and accumulators are THE model
    assert_replicas_identical(model, optimizer)
    ema = None
    if args.ema > 0:  # (after the broadcast: every rank's average starts from THE model)
        from nasrec_amd.utils.optim import WeightEMA
        ema = WeightEMA(model, args.ema)
    decay = None
    if args.decoupled_wd > 0:
        from nasrec_amd.utils.optim import DecoupledWeightDecay
        decay = DecoupledWeightDecay(model, args.decoupled_wd, args.no_reg_param_name)
    cowclip = build_cowclip(args, model)
    print(model)
    create_dir(args.logging_dir)
    with open(os.path.join(args.logging_dir, "configs_args.json"), "w") as f:
        json.dump(args.__dict__, f, indent=2)
    epoch_logs = []
    for epoch in range(args.num_epochs):
        # epoch index 1 is special-cased by the reference: 1000 steps, a test every 100 (main_train.py:206-207)
        logs = train_and_test_one_epoch(
            model, epoch, optimizer, lr_scheduler, train_loader, test_loader, loss_fn, l2_loss_fn, args.train_batch_size, args.gpu,
            display_interval=args.display_interval, test_interval=args.test_interval if epoch != 1 else 100,
            max_train_steps=steps_per_epoch if epoch != 1 else 1000, test_only_at_last_step=(args.test_only_at_last_step) == 1,
            tb_writer=writer, use_amp=False, grad_clip_value=5.0, ema=ema, decay=decay, cowclip=cowclip)
        epoch_logs.append(logs)
    print("Dumping logs to {}!".format(args.logging_dir))
    from nasrec_amd.utils.dist import world_info
    ckpt = os.path.join(args.logging_dir, "{}_checkpoint.pt".format(args.net))
    if world_info()[0] == 0:  # replicas are identical (broadcast at start, same global-batch update on every rank): rank 0 writes the artefacts
        save_model_checkpoint(model, ckpt, optimizer, ema=ema)
        dump_pickle_data(os.path.join(args.logging_dir, "train_test_logs.pickle"), epoch_logs)
    elif getattr(model, "_table_sharding", None):  # row-sharded tables: the whole-table state_dict is a collective
        save_model_checkpoint(model, None, optimizer, ema=ema)  # (tables and their accumulators are gathered: every rank takes part)
    return epoch_logs


def get_model(args):
    """main_train.py:233-272"""
    if args.net == "supernet":
        return SuperNet(sparse_input_size=_num_sparse_inputs_dict[args.dataset], num_blocks=7, ops_config=ops_config_lib["xlarge"],
                        use_layernorm=True, activation=args.activation, num_embeddings=_num_embedding_dict[args.dataset],
                        path_sampling_strategy="full-path", table_sharding=args.table_sharding,
                        matmul_precision=args.matmul_precision, table_dtype=TABLE_DTYPES[args.table_dtype])
    if args.net == "supernet-config":
        choice = load_json(args.supernet_config)
        print(choice)
        # the reference builds best-1shot sub-networks WITHOUT LayerNorm whatever the JSON says (main_train.py:262)
        return SuperNet(sparse_input_size=_num_sparse_inputs_dict[args.dataset], num_blocks=choice["num_blocks"],
                        ops_config=ops_config_lib[choice["config"]], use_layernorm=False, activation=args.activation,
                        num_embeddings=_num_embedding_dict[args.dataset], path_sampling_strategy="fixed-path", fixed=True,
                        fixed_choice=choice, table_sharding=args.table_sharding, matmul_precision=args.matmul_precision,
                        table_dtype=TABLE_DTYPES[args.table_dtype])
    raise NotImplementedError("Model {} is not implemented!".format(args.net))


def main(args):
    from nasrec_amd.utils.dist import init_from_env
    rank, world = init_from_env(args)  # torchrun: one process per GPU, args.gpu = the local rank
    check_table_dtype(args, world=world)
    check_cowclip(args, world=world)
    create_dir(args.logging_dir)
    print("Matmul precision: {}".format(args.matmul_precision))
    model = get_model(args).to(args.gpu)
    return train_and_eval_one_model(model, args)


def _decoupled_wd(text):
    v = float(text)
    if not v >= 0.0:
        raise argparse.ArgumentTypeError("--decoupled-wd %r is negative" % (text,))
    return v


def _ema_strength(text):
    v = float(text)
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError("--ema %r is not in [0, 1)" % (text,))
    return v


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", type=str, default="criteo-kaggle", help="Choice of datasets", choices=["criteo-kaggle", "avazu", "kdd"])
    p.add_argument("--root_dir", type=str, default="/home/tunhouzhang/local/datasets/criteo_kaggle_sharded")
    p.add_argument("--logging_dir", type=str, default=None, help="Directory to put loggings.")
    p.add_argument("--net", type=str, default="dlrm", help="Network backbone name", choices=["supernet", "supernet-config"])
    p.add_argument("--supernet_config", type=str, default=None, help="Supernet configuration.")
    p.add_argument("--wd", type=float, default=1e-8, help="L2 Weight decay")
    p.add_argument("--learning_rate", type=float, default=0.01, help="Learning rate")
    p.add_argument("--learning_rate_decay", type=float, default=0, help="Learning rate decay.")
    p.add_argument("--num_epochs", type=int, default=1, help="Number of epochs for training.")
    p.add_argument("--train_split", type=str, default="trainval", choices=["train", "trainval"],
                   help="Data split for training. Can be one of ['train', 'trainval']")
    p.add_argument("--validate_split", type=str, default="test", choices=["val", "test"],
                   help="Data split for validation (evaluation). Can be one of ['val', 'test']")
    p.add_argument("--train_batch_size", type=int, default=200, help="Training batch size.")
    p.add_argument("--test_batch_size", type=int, default=16368, help="Testing batch size.")
    p.add_argument("--optimizer", type=str, default="adagrad", help="Optimizer", choices=["adagrad", "sgd", "adam", "row-sparse-adam", "rowwise-adam", "rmsprop", "adam-adagrad-tables", "ds-optimizer"])
    p.add_argument("--table-lr-scale", dest="table_lr_scale", type=float, default=1.0,
                   help="--optimizer adam-adagrad-tables: the embedding tables' learning rate as a multiple of --learning_rate "
                        "(Adam's 1e-3 with 160 gives the tables 0.16)")
    p.add_argument("--table-eps", dest="table_eps", type=float, default=1e-2,
                   help="--optimizer adam-adagrad-tables: eps of the tables' Adagrad (> 0)")
    p.add_argument("--table-rowwise", dest="table_rowwise", action="store_true",
                   help="--optimizer adam-adagrad-tables: row-wise Adagrad on the tables — one accumulator per embedding row, fed the "
                        "mean of the row's squared gradient (1/16 of the element-wise state); refused with any other --optimizer")
    add_table_dtype_flags(p)
    # Criteo: train 36672495 / val 4584061 / test 4584061 / trainval 41256556; Avazu: 32343175 / 4042896 / 4042896 / 36386071;
    # KDD: 119711284 / 14963910 / 14963910 / 134675194
    p.add_argument("--train_limit", type=int, default=41256556, help="Maximum number of training examples.")
    p.add_argument("--test_limit", type=int, default=4584061, help="Maximum number of testing examples.")
    p.add_argument("--lr_schedule", default="cosine", help="Learning rate schedule", choices=["cosine", "constant", "constant-no-warmup"])
    p.add_argument("--display_interval", type=int, default=100, help="Interval to display tensorboard curve/training stats.")
    p.add_argument("--test_interval", type=int, default=2000, help="Testing intervals.")
    p.add_argument("--activation", type=str, default="relu", help="Activation function to use in this work.", choices=["relu", "silu"])
    p.add_argument("--no-reg-param-name", type=str, default=None, help="Name of the parameters that do not need to be regularized.")
    p.add_argument("--loss_function", type=str, default="bce", help="Loss function to perform the task.", choices=["bce"])
    p.add_argument("--test_only_at_last_step", type=int, default=0, help="Whether only test the last step.")
    p.add_argument("--ema", type=_ema_strength, default=0.0,
                   help="EMA strength in [0, 1); 0.9 / 0.99 / ... is recommended, 0 = off.  Keeps an exponential moving average of every "
                        "weight, s += (1 - ema) (w - s) after every optimizer step (utils/optim.WeightEMA); the tests run on the averaged "
                        "weights and the checkpoint carries them as ema_state_dict.  Inside the fused step with --optimizer adagrad / "
                        "row-sparse-adam / rowwise-adam / rmsprop / adam-adagrad-tables and no weight decay on the tables, on the torch route otherwise")
    p.add_argument("--decoupled-wd", dest="decoupled_wd", type=_decoupled_wd, default=0.0,
                   help="decoupled weight decay (the W of AdamW), 0 = off: before every optimizer step w *= 1 - lr * LAMBDA on the "
                        "parameters --wd would regularise (>= 2 dimensions, --no-reg-param-name left out) that have a gradient "
                        "(utils/optim.DecoupledWeightDecay).  Independent of --wd.  Inside the fused step with --optimizer adagrad / "
                        "row-sparse-adam / rowwise-adam / rmsprop / adam-adagrad-tables (embedding rows outside the batch pay lazily), on the torch route otherwise")
    add_cowclip_flag(p)
    p.add_argument("--gpu", type=int, default=None, help="GPU ID to use.")
    # not a reference flag: placement of the embedding tables under torchrun (nasrec_amd/sharded_tables.py)
    p.add_argument("--table-sharding", dest="table_sharding", type=str, default="none", choices=["none", "row"],
                   help="none: every rank holds whole tables (replicated, row gradients all-gathered; the fused step covers "
                        "--optimizer adagrad / adam / sgd with any --wd); row: every rank owns a row range of every table, ids / rows / "
                        "row gradients travel by all-to-all (tables that outgrow one GPU).  Row sharding needs the fused step's "
                        "--optimizer adagrad --wd 0")
    p.add_argument("--matmul-precision", dest="matmul_precision", type=str, default="highest", choices=["highest", "high", "medium"],
                   help="what the large-batch matrix products may feed the matrix cores (SuperNet(matmul_precision=...), as "
                        "torch.set_float32_matmul_precision): highest = fp32; high = bf16 x 3; medium = bf16. Tensors and accumulation stay fp32")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
