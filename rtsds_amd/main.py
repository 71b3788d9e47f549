"""CLI entry -- drop-in for the reference's main.py (flags main.py:233-260, config via
config.yaml, factories main.py:110-231, dispatch main.py:272-374) on the HIP path.

    python -m rtsds_amd.main [--config rtsds_amd/config.yaml] [--domain_adaptation]
                             [--model bisenet|deeplab] [--dataset cityscapes|gta5] [--seed 42]
                             [--self_training] [--distill] [--entropy_min]
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m rtsds_amd.main --domain_adaptation

Datasets (main.py:46-108): when the configured directories exist, the reference's readers
(rtsds_amd.datasets) feed the device-side transforms (rtsds_amd.transforms: antialiased
resize, normalize, augmentation, label clamp as HIP kernels); otherwise synthetic loaders of
the configured shapes are used (ImageNet-normalised 0-255 images, labels 0..19 with
19 = ignore), sharded per rank.  Deviations from the reference (documented in DESIGN.md): DA accepts a
DeepLab generator; validation accepts class_names / detailed_report.

--entropy_min (with --dataset gta5; config block training.entropy_minimisation, rtsds_amd/entmin.py):
the segmentation branch trains on labelled GTA5 batches and adds an unsupervised entropy penalty on
unlabelled Cityscapes train batches -- ADVENT's MinEnt, FDA's robust entropy or Maximum Squares.

--domain_adaptation with the config key training.domain_adaptation.discriminator_input: self_information
plays the adversarial game on ADVENT's self-information maps -p log p / log c (AdvEnt) instead of the
probabilities (softmax, the default: the reference's AdaptSegNet form); train.da_step's d_input.
"""
import argparse
import os
from collections import namedtuple

import numpy as np
import torch
import yaml

from . import losses, optim
from .functional import ENTROPY_PENALTIES
from .models.bisenet import build_bisenet
from .models.deeplabv2 import deeplabv2
from .models.domain_shift.adversarial.model import DomainDiscriminator, TinyDomainDiscriminator
from .runtime import set_compute_dtype
from .train import D_INPUTS, adversarial_train, train
from .utils import dist_env, forModel
from .validation import val, val_GTA5


def criterion_weight(loss_config, num_classes=None):
    """The optional ``weight`` key of a CrossEntropy criterion block: None, a list of
    ``num_classes`` finite non-negative numbers (taken as is), or one of losses.WEIGHT_MODES
    (computed from the training labels before training: install_class_weights).  Anything else
    raises at start-up."""
    w = loss_config.get("weight")
    if w is None:
        return None
    if isinstance(w, str):
        if w not in losses.WEIGHT_MODES:
            raise ValueError(f"rtsds_amd: criterion.weight must be a list of class weights or one of "
                             f"{', '.join(repr(m) for m in losses.WEIGHT_MODES)}, got {w!r}")
        return w
    if not isinstance(w, (list, tuple)):
        raise ValueError(f"rtsds_amd: criterion.weight must be a list of class weights or a mode name, got {w!r}")
    if num_classes is not None and len(w) != num_classes:
        raise ValueError(f"rtsds_amd: criterion.weight has {len(w)} entries for {num_classes} classes")
    return list(w)


def optimzer_loss_loader(model, optimizer_config, loss_config, num_classes=None):
    """main.py:110-136 with the HIP-backed Adam / SGD and losses.  A CrossEntropy criterion takes
    the list form of ``weight`` directly (moved to the model's device); a mode name is left on the
    criterion as ``weight_mode`` for install_class_weights."""
    if optimizer_config["name"] == "Adam":
        optimizer = optim.Adam(model.parameters(), lr=optimizer_config["lr"],
                               weight_decay=optimizer_config.get("weight_decay", 0))
    elif optimizer_config["name"] == "SGD":
        optimizer = optim.SGD(model.parameters(), lr=optimizer_config["lr"],
                              momentum=optimizer_config["momentum"])
    else:
        raise ValueError("Invalid optimizer name. Please select Adam or SGD")
    if loss_config["name"] == "CrossEntropy":
        w = criterion_weight(loss_config, num_classes)
        loss = losses.CrossEntropyLoss(weight=None if isinstance(w, str) else w, ignore_index=loss_config.get("ignore_index"))
        loss.weight_mode = w if isinstance(w, str) else None
        if loss.weight is not None:
            loss.to(next(model.parameters()).device)
    elif loss_config["name"] == "BCEWithLogits":
        loss = losses.BCEWithLogitsLoss()
    else:
        raise ValueError("Invalid loss name. Please select CrossEntropy or BCEWithLogits")
    return optimizer, loss


def _generator(model_cfg, name):
    if name == "bisenet":
        b = model_cfg["bisenet"]
        return build_bisenet.BiSeNet(num_classes=b["num_classes"], context_path=b["backbone"])
    if name == "deeplab":
        d = model_cfg["deeplab"]
        return deeplabv2.get_deeplab_v2(d["num_classes"], pretrain=d.get("pretrain", False),
                                        pretrain_model_path=d.get("pretrain_model_path"))
    raise ValueError("Invalid model name. Please select deeplab or bisenet")


def model_loader(config, is_adversarial, model_name):
    """main.py:138-231.  Models are moved to the device BEFORE the optimizers are built so
    the fused Adam's arena is created on the GPU."""
    model_cfg = config.model
    if is_adversarial:
        adv = model_cfg["adversarial_model"]
        gen = forModel(_generator(model_cfg, adv["generator"]["name"]), config.device)
        g_opt, g_loss = optimzer_loss_loader(gen, adv["generator"]["optimizer"], adv["generator"]["criterion"],
                                             model_cfg[adv["generator"]["name"]]["num_classes"])
        g_hp = {"gen_init_lr": adv["generator"]["optimizer"]["lr"], "gen_power": adv["generator"]["power_lr_factor"]}
        dcfg = adv["discriminator"]
        dis = (TinyDomainDiscriminator(num_classes=dcfg["input_channels"]) if dcfg["name"] == "tiny"
               else DomainDiscriminator(num_classes=dcfg["input_channels"]))
        dis = forModel(dis, config.device)
        d_opt, d_loss = optimzer_loss_loader(dis, dcfg["optimizer"], dcfg["criterion"])
        d_hp = {"dis_init_lr": dcfg["optimizer"]["lr"], "dis_power": dcfg["power_lr_factor"]}
        return (gen, g_opt, g_loss, g_hp), (dis, d_opt, d_loss, d_hp)
    cfg = model_cfg["deeplab" if model_name == "deeplab" else "bisenet"]
    model = forModel(_generator(model_cfg, model_name), config.device)
    opt, loss = optimzer_loss_loader(model, cfg["optimizer"], cfg["criterion"], cfg["num_classes"])
    return model, opt, loss, {"init_lr": cfg["optimizer"]["lr"], "power": cfg["power_lr_factor"]}


def install_class_weights(criterion, loader, num_classes, class_names, device):
    """A criterion configured with ``weight: "inverse_log" | "median_frequency"``: one sweep over
    the (source) training loader's labels on the device (losses.class_statistics, summed over
    data-parallel ranks), the weights from the exact counts (losses.class_weights), logged beside
    the class names and installed.  Any other criterion is left alone.  Returns the weights."""
    mode = getattr(criterion, "weight_mode", None)
    if mode is None:
        return None
    count, support = losses.class_statistics(loader, num_classes, criterion.ignore_index, device)
    w = losses.class_weights(count, support, mode)
    names = list(class_names or [])
    print(f"Class weights ({mode}):")
    for k in range(num_classes):
        print(f"  {names[k] if k < len(names) else k}: {w[k]:.4f}  ({int(count[k])} pixels)")
    criterion.set_weight(w)
    criterion.to(device)
    return w


class SyntheticLoader:
    """Fixed synthetic batches of the configured size (list semantics: len / iter / index)."""

    def __init__(self, batches, batch_size, size, num_classes, seed):
        h, w = size
        g = torch.Generator().manual_seed(seed)
        mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        self.data = []
        for _ in range(batches):
            x = (torch.randint(0, 256, (batch_size, 3, h, w), generator=g).float() - mean) / std
            y = torch.randint(0, num_classes + 1, (batch_size, 1, h, w), generator=g)
            self.data.append((x, y))

    def __len__(self):
        return len(self.data)

    def __iter__(self):
        return iter(self.data)


HISTOGRAM_BANK_CAPACITY = 64  # augmentation.HistogramMatching.bank, when absent


def build_histogram_bank(dataset, capacity, device="cuda"):
    """The target histograms augmentation HistogramMatching draws from: the raw images
    ``dataset[i][0]`` at transforms.bank_indices(len(dataset), capacity) -- an even spread, the
    same on every rank -- moved to the device and counted there (3 KB kept per image)."""
    from . import transforms as T
    bank = T.HistogramBank(capacity, device)
    for i in T.bank_indices(len(dataset), capacity):
        bank.add([dataset[i][0].to(device)])
    return bank


SPECTRUM_BANK_CAPACITY = 64  # augmentation.FourierAdaptation.bank, when absent


def build_spectrum_bank(dataset, capacity=SPECTRUM_BANK_CAPACITY, b=7, device="cuda"):
    """The target amplitudes augmentation FourierAdaptation draws from: the band |u|, |v| <= b of
    the raw images ``dataset[i][0]`` at transforms.bank_indices(len(dataset), capacity), the same
    spread as build_histogram_bank's.  The images keep their own size: an entry is |F| / (h w) at
    the image's own integer frequencies (cycles per image), 12 (2b+1)(b+1) bytes each."""
    from . import transforms as T
    bank = T.SpectrumBank(capacity, b, device)
    for i in T.bank_indices(len(dataset), capacity):
        bank.add([dataset[i][0].to(device)])
    return bank


def real_datasets_loader(config, is_augmented, device="cuda"):
    """main.py:60-108 on the device pipeline: the reference's readers (PNG decode on CPU
    DataLoader workers) deliver raw uint8 samples, batches go to HBM and through the
    torchvision-equivalent HIP transforms (rtsds_amd.transforms); under data parallelism each
    rank reads a disjoint shard of the training sets (DistributedSampler, a new permutation per
    iterator -- transforms.DeviceLoader advances its epoch); validation reads the whole set."""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler

    from . import transforms as T
    from .datasets import GTA5, CityScapes
    cs, gta = config.data["cityscapes"], config.data["gta5_modified"]
    cs_size, gta_size = T.parse_size(cs["image_size"]), T.parse_size(gta["image_size"])
    rank, _, world = dist_env()

    def loader(ds, bs, workers, shuffle, shard=True):
        sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle) \
            if world > 1 and shard else None
        return DataLoader(ds, batch_size=bs, shuffle=shuffle and sampler is None, sampler=sampler, pin_memory=False,
                          num_workers=workers, collate_fn=T.collate_raw)

    city_img = T.ImagePipeline(cs_size)
    city_lbl = T.LabelPipeline(cs_size, clamp=(0, cs["num_classes"]))
    train_ds = CityScapes(cs["segmentation_train_dir"], cs["images_train_dir"])
    bank = None
    if is_augmented and "HistogramMatching" in config.augmentation:  # GTA5 colours towards Cityscapes train
        capacity = (config.augmentation["HistogramMatching"] or {}).get("bank", HISTOGRAM_BANK_CAPACITY)
        bank = build_histogram_bank(train_ds, capacity, device)
    spectrum_bank = None
    if is_augmented and "FourierAdaptation" in config.augmentation:  # GTA5 low frequencies towards Cityscapes train
        c = config.augmentation["FourierAdaptation"] or {}
        # the band of the configured GTA5 frame; the transform checks every decoded image against it
        b = T.FourierAdaptation(None, beta=c.get("beta", 0.01)).band(*gta_size)
        spectrum_bank = build_spectrum_bank(train_ds, c.get("bank", SPECTRUM_BANK_CAPACITY), b, device)
    gta_img = T.ImagePipeline(gta_size, augment=T.augmentation_loader(config, 0.5, bank=bank, spectrum_bank=spectrum_bank)
                              if is_augmented else None)
    gta_lbl = T.LabelPipeline(gta_size)
    val_ds = CityScapes(cs["segmentation_val_dir"], cs["images_val_dir"])
    gta_ds = GTA5(gta["images_dir"], gta["segmentation_dir"], None, None)
    return (T.DeviceLoader(loader(train_ds, cs["batch_size"], cs["num_workers"], True), city_img, city_lbl, device),
            # validation is not sharded: a DistributedSampler pads shards with duplicates and
            # the confusion histogram is per process, so every rank evaluates the full val set
            # and reports the reference's full-set mIoU
            T.DeviceLoader(loader(val_ds, cs["batch_size"], cs["num_workers"], False, shard=False),
                           city_img, city_lbl, device),
            T.DeviceLoader(loader(gta_ds, gta["batch_size"], gta["num_workers"], True), gta_img, gta_lbl, device))


def datasets_loader(config, is_augmented):
    """main.py:60-108: the dataset directories of config.yaml through the device pipeline when
    they exist, else synthetic loaders of the configured shapes."""
    cs, gta = config.data["cityscapes"], config.data["gta5_modified"]
    present = os.path.isdir(cs["images_train_dir"]) and os.path.isdir(gta["images_dir"])
    if present:
        return real_datasets_loader(config, is_augmented, config.device)
    rank = dist_env()[0]
    nb = config.data.get("synthetic_batches", 4)
    size = lambda s: [int(v) for v in str(s).split(",")]  # noqa: E731
    city = SyntheticLoader(nb, cs["batch_size"], size(cs["image_size"]), cs["num_classes"], 1000 + 2 * rank)
    val_l = SyntheticLoader(1, cs["batch_size"], size(cs["image_size"]), cs["num_classes"], 7)
    gta5 = SyntheticLoader(nb, gta["batch_size"], size(gta["image_size"]), gta["num_classes"], 2000 + 2 * rank)
    return city, val_l, gta5


def ordered_target_loader(config, train_dl):
    """The target-train loader self-training sweeps: it must replay the same batches in the same
    order on every iteration (selftrain.PseudoLabelLoader).  Synthetic data: ``train_dl`` itself
    (SyntheticLoader is a fixed list).  Real data: Cityscapes train through the device pipeline,
    not shuffled and not augmented; under data parallelism each rank reads its own fixed shard
    (DistributedSampler(shuffle=False))."""
    cs, gta = config.data["cityscapes"], config.data["gta5_modified"]
    if not (os.path.isdir(cs["images_train_dir"]) and os.path.isdir(gta["images_dir"])):
        return train_dl
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler

    from . import transforms as T
    from .datasets import CityScapes
    size = T.parse_size(cs["image_size"])
    rank, _, world = dist_env()
    ds = CityScapes(cs["segmentation_train_dir"], cs["images_train_dir"])
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=False) if world > 1 else None
    dl = DataLoader(ds, batch_size=cs["batch_size"], shuffle=False, sampler=sampler, pin_memory=False,
                    num_workers=cs["num_workers"], collate_fn=T.collate_raw)
    return T.DeviceLoader(dl, T.ImagePipeline(size), T.LabelPipeline(size, clamp=(0, cs["num_classes"])), config.device)


SELF_TRAINING_KEYS = ("rounds", "epochs", "portion", "portion_step", "cap", "bins", "lr_scale", "scales", "flip")
SELF_TRAINING_MODES = ("offline", "online")
ONLINE_SELF_TRAINING_KEYS = ("epochs", "lr_scale", "ema_decay", "threshold")  # with mode: online


def self_training_config(config):
    """The training.self_training block (commented out in the shipped config.yaml), complete."""
    st = config.training.get("self_training")
    if st is None:
        raise RuntimeError("rtsds_amd: --self_training needs the config block training.self_training "
                           f"(keys: {', '.join(SELF_TRAINING_KEYS)}; or mode: online with "
                           f"{', '.join(ONLINE_SELF_TRAINING_KEYS)}); config.yaml ships it commented out")
    mode = st.get("mode", "offline")  # optional: absent = the offline, class-balanced form
    if mode not in SELF_TRAINING_MODES:
        raise RuntimeError(f"rtsds_amd: training.self_training.mode must be one of "
                           f"{', '.join(repr(m) for m in SELF_TRAINING_MODES)}, got {mode!r}")
    missing = [k for k in (ONLINE_SELF_TRAINING_KEYS if mode == "online" else SELF_TRAINING_KEYS) if k not in st]
    if missing:
        raise RuntimeError(f"rtsds_amd: training.self_training lacks {', '.join(missing)}")
    if st.get("mix") not in (None, "classmix"):  # optional: absent = pseudo-labels alone
        raise RuntimeError(f"rtsds_amd: training.self_training.mix must be 'classmix' when given, got {st['mix']!r}")
    return st


DISTILLATION_KEYS = ("teacher_model", "teacher_weights", "temperature", "weight")
DISTILLATION_MODELS = ("deeplab", "bisenet")


def distillation_config(config):
    """The training.distillation block (commented out in the shipped config.yaml), complete."""
    kd = config.training.get("distillation")
    if kd is None:
        raise RuntimeError("rtsds_amd: --distill needs the config block training.distillation "
                           f"(keys: {', '.join(DISTILLATION_KEYS)}); config.yaml ships it commented out")
    missing = [k for k in DISTILLATION_KEYS if k not in kd]
    if missing:
        raise RuntimeError(f"rtsds_amd: training.distillation lacks {', '.join(missing)}")
    if kd["teacher_model"] not in DISTILLATION_MODELS:
        raise RuntimeError(f"rtsds_amd: training.distillation.teacher_model must be one of "
                           f"{', '.join(repr(m) for m in DISTILLATION_MODELS)}, got {kd['teacher_model']!r}")
    for k, ok in (("temperature", lambda v: v > 0), ("weight", lambda v: v >= 0)):
        v = kd[k]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or not ok(v):
            raise RuntimeError(f"rtsds_amd: training.distillation.{k} must be a "
                               f"{'positive' if k == 'temperature' else 'non-negative'} number, got {v!r}")
    if not isinstance(kd["teacher_weights"], str) or not kd["teacher_weights"]:
        raise RuntimeError("rtsds_amd: training.distillation.teacher_weights must be the path of a state_dict")
    return kd


def build_distiller(config, kd):
    """The frozen teacher of the training.distillation block, built as predict.build_model builds
    its model (DeepLab's ``pretrain`` off, the state_dict read with weights_only=True, nothing
    fetched), as a distill.Distiller."""
    from .distill import Distiller
    from .predict import build_model
    if not os.path.isfile(kd["teacher_weights"]):
        raise RuntimeError(f"rtsds_amd: training.distillation.teacher_weights {kd['teacher_weights']} does not exist")
    teacher = build_model(config, kd["teacher_model"], kd["teacher_weights"])
    return Distiller(teacher, temperature=kd["temperature"], weight=kd["weight"])


ENTROPY_MINIMISATION_KEYS = ("penalty", "weight", "eta")


def entropy_minimisation_config(config):
    """The training.entropy_minimisation block (commented out in the shipped config.yaml), complete."""
    em = config.training.get("entropy_minimisation")
    if em is None:
        raise RuntimeError("rtsds_amd: --entropy_min needs the config block training.entropy_minimisation "
                           f"(keys: {', '.join(ENTROPY_MINIMISATION_KEYS)}); config.yaml ships it commented out")
    missing = [k for k in ENTROPY_MINIMISATION_KEYS if k not in em]
    if missing:
        raise RuntimeError(f"rtsds_amd: training.entropy_minimisation lacks {', '.join(missing)}")
    if em["penalty"] not in ENTROPY_PENALTIES:
        raise RuntimeError(f"rtsds_amd: training.entropy_minimisation.penalty must be one of "
                           f"{', '.join(repr(p) for p in ENTROPY_PENALTIES)}, got {em['penalty']!r}")
    for k, ok in (("eta", lambda v: v > 0), ("weight", lambda v: v >= 0)):
        v = em[k]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or not ok(v):
            raise RuntimeError(f"rtsds_amd: training.entropy_minimisation.{k} must be a "
                               f"{'positive' if k == 'eta' else 'non-negative'} number, got {v!r}")
    return em


def discriminator_input_config(config):
    """training.domain_adaptation.discriminator_input: what the discriminator sees of the generator's
    output, ``softmax`` (absent: the same) or ``self_information`` (AdvEnt); train.da_step's d_input."""
    v = config.training["domain_adaptation"].get("discriminator_input", "softmax")
    if not isinstance(v, str) or v not in D_INPUTS:
        raise RuntimeError(f"rtsds_amd: training.domain_adaptation.discriminator_input must be one of "
                           f"{', '.join(D_INPUTS)}, got {v!r}")
    return v


def self_train_online(config, st, model, optimizer, criterion, init_lr, power, lr_decay_iter, target_dl, validate,
                      callbacks, source_dl, model_name):
    """Online (mean-teacher) self-training, ``mode: online``: a second model of the branch's
    architecture becomes the EMA teacher of ``model`` (ema.EMATeacher, decay ``ema_decay``), the
    target loader -- in whatever order, shuffled and augmented included -- is wrapped in
    selftrain.TeacherLoader (labels made per batch by the teacher above the confidence
    ``threshold``; with ``mix: classmix`` mixed with the labelled ``source_dl``), and ``epochs``
    epochs of train.train run on it, the teacher updated after every step; lr as in the offline
    form.  ``validate(epoch)`` validates the student after every epoch.  Returns the teacher."""
    from . import selftrain
    from .ema import EMATeacher
    ignore_index = getattr(criterion, "ignore_index", None)
    teacher = EMATeacher(model, model_loader(config, False, model_name)[0], optimizer, decay=st["ema_decay"])
    loader = selftrain.TeacherLoader(target_dl, teacher, threshold=st["threshold"], ignore_index=ignore_index,
                                     bins=st.get("bins", 1024), source_loader=source_dl if st.get("mix") else None)
    max_iter = st["epochs"] * len(loader)
    for epoch in range(st["epochs"]):
        train(model=model, optimizer=optimizer, criterion=criterion, train_loader=loader, epoch=epoch,
              init_lr=init_lr * st["lr_scale"], lr_decay_iter=lr_decay_iter, power=power, max_iter=max_iter,
              callbacks=callbacks, device=config.device)
        kept = float(loader.kept_sum) / max(1, loader.pixels) if loader.kept_sum is not None else 0.0
        print(f"Self-training (online) epoch {epoch + 1}: threshold {loader.tbin_value / loader.bins:.4f}, "
              f"labelled share {kept:.3f}, teacher updates {teacher.updates}")
        validate(epoch)
    return teacher


def self_train(config, st, model, optimizer, criterion, init_lr, power, lr_decay_iter, num_classes, target_dl,
               validate, callbacks, source_dl=None, model_name="bisenet"):
    """Class-balanced self-training after the normal run (rtsds_amd.selftrain): per round one
    sweep over the ordered target loader (generate), global per-class thresholds for the round's
    portion (class_thresholds), then ``epochs`` epochs of train.train on the thresholded labels
    with the branch's model, optimizer and criterion; lr = init_lr * lr_scale, poly-decayed over
    all self-training iterations.  ``validate(epoch)`` runs after every epoch.  With the optional
    key ``mix: classmix`` every batch is mixed with the next batch of the labelled ``source_dl``
    (selftrain.ClassMixLoader) instead of carrying pseudo-labels alone.  With ``mode: online``
    none of that runs: self_train_online (``model_name``: the architecture of ``model``, for the
    teacher) labels every batch with an EMA teacher instead."""
    from . import selftrain
    ignore_index = getattr(criterion, "ignore_index", None)
    if ignore_index is None:
        raise RuntimeError("rtsds_amd: --self_training needs a criterion with ignore_index (CrossEntropy)")
    mix = st.get("mix")  # self_training_config: None or "classmix"
    if mix is not None and source_dl is None:
        raise RuntimeError("rtsds_amd: training.self_training.mix: classmix needs the labelled source loader")
    if st.get("mode") == "online":
        return self_train_online(config, st, model, optimizer, criterion, init_lr, power, lr_decay_iter, target_dl,
                                 validate, callbacks, source_dl, model_name)
    loader = ordered_target_loader(config, target_dl)
    max_iter = st["rounds"] * st["epochs"] * len(loader)
    for rnd in range(st["rounds"]):
        labels = selftrain.generate(model, loader, num_classes, bins=st["bins"], scales=tuple(st["scales"]),
                                    flip=bool(st["flip"]), device=config.device)
        portion = min(1.0, st["portion"] + rnd * st["portion_step"])
        tbin = selftrain.class_thresholds(labels.hist, portion, st["cap"])
        kept = selftrain.kept_fraction(labels, tbin)
        print(f"Self-training round {rnd + 1}: portion {portion:.3f}, thresholds "
              f"{[round(int(b) / st['bins'], 3) for b in tbin]}, kept {[round(float(k), 3) for k in kept]}")
        if mix is None:
            pseudo = selftrain.PseudoLabelLoader(loader, labels, tbin, ignore_index)
        else:
            pseudo = selftrain.ClassMixLoader(loader, source_dl, labels, tbin, ignore_index)
        for e in range(st["epochs"]):
            epoch = rnd * st["epochs"] + e
            train(model=model, optimizer=optimizer, criterion=criterion, train_loader=pseudo, epoch=epoch,
                  init_lr=init_lr * st["lr_scale"], lr_decay_iter=lr_decay_iter, power=power, max_iter=max_iter,
                  callbacks=callbacks, device=config.device)
            validate(epoch)


def argumnet_parser(argv=None):
    p = argparse.ArgumentParser(description="Semantic Segmentation and Domain Adaptation (MI355X)")
    p.add_argument("--config", type=str, default=os.path.join(os.path.dirname(__file__), "config.yaml"))
    p.add_argument("--dataset", type=str, default="cityscapes")
    p.add_argument("--augmented", action="store_true")
    p.add_argument("--domain_adaptation", action="store_true",
                   help="adversarial training against a domain discriminator; the config key "
                        "training.domain_adaptation.discriminator_input chooses what it sees: softmax "
                        "(AdaptSegNet, the default) or self_information (AdvEnt)")
    p.add_argument("--model", type=str, default="bisenet")
    p.add_argument("--wandb", action="store_true")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--self_training", action="store_true",
                   help="self-training on the target set after the normal run: class-balanced sweeps, or "
                        "with mode: online an EMA teacher per batch (config block training.self_training)")
    p.add_argument("--distill", action="store_true",
                   help="segmentation branch only: add a frozen teacher's soft targets to the loss "
                        "(config block training.distillation)")
    p.add_argument("--entropy_min", action="store_true",
                   help="segmentation branch only, with --dataset gta5: add an entropy penalty on unlabelled "
                        "Cityscapes batches to the loss (config block training.entropy_minimisation)")
    return p.parse_args(argv)


def set_seed(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)


def load_config(path):
    with open(path) as f:
        cfg = yaml.safe_load(f)
    return namedtuple("Config", cfg.keys())(*cfg.values())


def main(argv=None):
    args = argumnet_parser(argv)
    set_seed(args.seed)
    config = load_config(args.config)
    set_compute_dtype(torch.bfloat16 if getattr(config, "precision", "fp32") == "bf16" else torch.float32)
    st = self_training_config(config) if args.self_training else None
    if args.distill and args.domain_adaptation:
        raise RuntimeError("rtsds_amd: --distill applies to the segmentation branch only, not with --domain_adaptation")
    if args.entropy_min and args.domain_adaptation:
        raise RuntimeError("rtsds_amd: --entropy_min applies to the segmentation branch only, not with --domain_adaptation")
    if args.entropy_min and args.distill:
        raise RuntimeError("rtsds_amd: --entropy_min and --distill are separate loops; give one of them")
    if args.entropy_min and args.dataset != "gta5":
        raise RuntimeError("rtsds_amd: --entropy_min needs --dataset gta5: the labelled source is GTA5 and the target is "
                           "the Cityscapes train set (else source and target would be the same set)")
    kd = distillation_config(config) if args.distill else None
    em =entropy_minimisation_config(config) if args.entropy_min else None
    d_input = discriminator_input_config(config) if args.domain_adaptation else None
    train_dl, val_dl, gta_dl = datasets_loader(config, args.augmented)
    target_dl = train_dl
    callbacks = []
    if args.domain_adaptation:
        (g, g_opt, g_loss, g_hp), (d, d_opt, d_loss, d_hp) = model_loader(config, True, args.model)
        t = config.training["domain_adaptation"]
        install_class_weights(g_loss, gta_dl, t["num_classes"], config.meta["class_names"], config.device)
        adversarial_train(iterations=t["iterations"], epochs=t["epochs"], lambda_=t["lambda"], generator=g,
                          discriminator=d, generator_optimizer=g_opt, discriminator_optimizer=d_opt,
                          generator_loss=g_loss, discriminator_loss=d_loss, source_dataloader=gta_dl,
                          target_dataloader=train_dl, gen_init_lr=g_hp["gen_init_lr"],
                          dis_init_lr=d_hp["dis_init_lr"], lr_decay_iter=t["lr_decay_iter"],
                          gen_power=g_hp["gen_power"], dis_power=d_hp["dis_power"],
                          num_classes=t["num_classes"], class_names=config.meta["class_names"],
                          val_loader=val_dl, do_validation=t["do_validation"], when_print=t["when_print"],
                          callbacks=callbacks, device=config.device, d_input=d_input)
        if st is not None:
            self_train(config, st, g, g_opt, g_loss, g_hp["gen_init_lr"], g_hp["gen_power"], t["lr_decay_iter"],
                       t["num_classes"], target_dl,
                       lambda epoch: val_GTA5(epoch, g, val_dl, t["num_classes"], config.meta["class_names"],
                                              callbacks, device=config.device), callbacks, source_dl=gta_dl,
                       model_name=config.model["adversarial_model"]["generator"]["name"])
    else:
        if args.dataset == "gta5":
            train_dl = gta_dl
        model, opt, crit, hp = model_loader(config, False, args.model)
        t = config.training["segmentation"]
        install_class_weights(crit, train_dl, t["num_classes"], config.meta["class_names"], config.device)
        max_iter = t["epochs"] * len(train_dl)
        if kd is not None:
            from . import distill
            distiller = build_distiller(config, kd)
        if em is not None:
            from . import entmin
            minimiser = entmin.EntropyMinimiser(penalty=em["penalty"], eta=em["eta"], weight=em["weight"])
        for epoch in range(t["epochs"]):
            if em is not None:
                entmin.train(model=model, optimizer=opt, criterion=crit, train_loader=train_dl, epoch=epoch,
                             init_lr=hp["init_lr"], lr_decay_iter=t["lr_decay_iter"], power=hp["power"],
                             max_iter=max_iter, callbacks=callbacks, device=config.device, target_loader=target_dl,
                             minimiser=minimiser)
            elif kd is not None:
                distill.train(model=model, optimizer=opt, criterion=crit, train_loader=train_dl, epoch=epoch,
                              init_lr=hp["init_lr"], lr_decay_iter=t["lr_decay_iter"], power=hp["power"],
                              max_iter=max_iter, callbacks=callbacks, device=config.device, distiller=distiller)
            else:
                train(model=model, optimizer=opt, criterion=crit, train_loader=train_dl, epoch=epoch,
                      init_lr=hp["init_lr"], lr_decay_iter=t["lr_decay_iter"], power=hp["power"],
                      max_iter=max_iter, callbacks=callbacks, device=config.device)
            val(epoch=epoch, model=model, val_loader=val_dl, num_classes=t["num_classes"],
                class_names=config.meta["class_names"], detailed_report=True, device=config.device,
                callbacks=callbacks, scales=t.get("eval_scales"), flip=bool(t.get("eval_flip", False)))
        if st is not None:
            self_train(config, st, model, opt, crit, hp["init_lr"], hp["power"], t["lr_decay_iter"], t["num_classes"],
                       target_dl,
                       lambda epoch: val(epoch=epoch, model=model, val_loader=val_dl, num_classes=t["num_classes"],
                                         class_names=config.meta["class_names"], detailed_report=True,
                                         device=config.device, callbacks=callbacks, scales=t.get("eval_scales"),
                                         flip=bool(t.get("eval_flip", False))), callbacks, source_dl=gta_dl,
                       model_name=args.model)


if __name__ == "__main__":
    main()
