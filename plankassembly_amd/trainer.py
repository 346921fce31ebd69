"""Trainer surface of the reference (trainer_complete.py / trainer_visible.py / trainer_sideface.py)
for the MI355X hot path, without Lightning / detectron2 / torchmetrics / jsonargparse (none of
them is installed in this image): same class, same hook names (Lightning 1.7: ``training_step``,
``validation_step``, ``validation_epoch_end``, ``test_step``, ``test_epoch_end``,
``configure_optimizers``, ``*_dataloader``), same YAML config files, same CLI shape
(``fit`` / ``test``, ``--config``, ``--ckpt_path``, ``--trainer.<key> value``).

What differs is underneath: ``self.model`` is the HIP-backed PlankModel, the optimizer is the fused
Adam over the flat parameter buffer, and the ``ddp`` strategy is one process per GPU with the
segmented RCCL gradient exchange of ``plankassembly_amd.distributed`` (launch with
``python -m torch.distributed.run --nproc-per-node N trainer_complete.py fit --config ...``).
Checkpoints are Lightning-shaped (``state_dict`` with the ``model.`` prefix + ``hyper_parameters``),
so the reference's published checkpoints load and ours load in the reference.
"""
from __future__ import annotations

import contextlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

from .config import CfgNode, load_cli_config
from .data import SynthSpec, synth_sample
from .datasets import LineDataset, SidefaceDataset, extract_mode, parse_splits_list, render_mode  # noqa: F401  (parse_splits_list re-exported)
from .metric import DevicePlankScorer, PlankScorer, planks_of_row, valid_planks
from .distributed import allreduce_metric_sums
from .models import build_model


class SyntheticDrawings(torch.utils.data.Dataset):
    """Seeded synthetic samples with the reference dataloader's tensor layout (the real
    PlankAssembly dataset needs network access)."""

    def __init__(self, n, spec: SynthSpec, seed=2022):
        self.n, self.spec, self.seed = n, spec, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = np.random.default_rng(self.seed + i)
        s = synth_sample(rng, self.spec)
        out = {"name": f"synth_{self.seed}_{i:06d}"}
        out.update({k: torch.from_numpy(np.asarray(v)) for k, v in s.items()})
        return out


class _Logger:
    def __init__(self, root="lightning_logs"):
        v = 0
        while os.path.exists(os.path.join(root, f"version_{v}")):
            v += 1
        self.log_dir = os.path.join(root, f"version_{v}")
        self.history = []

    def log(self, name, value, step):
        self.history.append((step, name, float(value)))


class Trainer(torch.nn.Module):
    """reference trainer_complete.py:19-129."""

    with_type = True
    default_lines = (8, 299)
    dataset_cls = LineDataset
    device_kind = "line"                       # plankassembly_amd.device_data.pack_infos(kind=...)
    train_augmentation = True

    def __init__(self, hparams):
        super().__init__()
        self.hparams_dict = dict(hparams)
        cfg = CfgNode(hparams)
        self.cfg = cfg
        self.model = build_model(cfg)
        # DEVICE_METRIC: true (opt-in, like DEVICE_DATASET): validation / test drawings are matched on the GPU, one launch per batch
        # (metric.DevicePlankScorer); the logged means and the pred_jsons are those of the host path, bit for bit
        self.device_metric = bool(cfg.get("DEVICE_METRIC", False))
        self.scorer = DevicePlankScorer(cfg.THRESHOLD, cfg.TOKEN.END) if self.device_metric else PlankScorer(cfg.THRESHOLD)
        self.matcher, self.criterion = self.scorer.matcher, self.scorer.criterion      # the reference's attribute names
        self.logger = None
        self.global_step = 0
        self._logged = {}
        self.optimizer_kwargs = {}             # FusedAdam's guard arguments, from the `trainer:` block (optimizer_options)
        self.recipe = recipe_options(self.hparams_dict)  # weight decay / LR schedule / EMA keys of the hparams, validated
        self.seq_train = seq_train_options(self.hparams_dict)   # the SEQ_TRAIN block, validated; None: plain NLL steps only
        self.extract_sideface = extract_option(self.hparams_dict)      # DATA.EXTRACT_SIDEFACE, validated (sideface kind only)
        self.render_drawings = render_option(self.hparams_dict)        # DATA.RENDER_DRAWINGS, validated
        self._train_reward = None
        # REPROJECTION_METRIC: true (opt-in): validation / test also average the reprojection F1 of the returned programs - how well
        # their rendered three views match the given drawings (PlankModel.reprojection), on the device
        self.reprojection_metric = reprojection_option(self.hparams_dict, self.device_kind, cfg.DATA.NUM_OUTPUT_DOF)
        self._reprojection_sums = None         # float64 [2] on the device: the sum of F1 and the number of drawings
        # VOLUME_METRIC: true (opt-in): validation / test also average shape IoU / precision / recall against the ground truth and the
        # self-overlap of the returned programs (PlankModel.volume), on the device; any input kind
        self.volume_metric = volume_option(self.hparams_dict, cfg.DATA.NUM_OUTPUT_DOF)
        self._volume_sums = None               # float64 [5] on the device: the four sums and the number of drawings

    # ------------------------------------------------------------------ logging (self.log of Lightning)
    def log(self, name, value, **kw):
        v = float(value)
        self._logged[name] = v
        if self.logger is not None:
            self.logger.log(name, v, self.global_step)

    # ------------------------------------------------------------------ data
    def _spec(self):
        d = self.cfg.DATA
        hi = min(self.default_lines[1], (d.MAX_INPUT_LENGTH - 2) // d.NUM_INPUT_DOF)
        return SynthSpec(d.MAX_INPUT_LENGTH, d.MAX_OUTPUT_LENGTH, (min(self.default_lines[0], hi), hi),
                         (2, (d.MAX_OUTPUT_LENGTH - 1) // d.NUM_OUTPUT_DOF), self.with_type)

    def _dataset(self, split_key, n_default, seed, augmentation):
        """The reference's dataset over ``ROOT`` + split file when both exist on disk (trainer_complete.py:35-61),
        else the seeded synthetic generator (there is no network to fetch the real dataset here)."""
        split = self.cfg.get(split_key)
        root = str(self.cfg.get("ROOT", ""))
        have_split = bool(split) and all(os.path.exists(s) for s in str(split).split())
        if have_split and os.path.isdir(root):
            return self.dataset_cls(root, parse_splits_list(split), self.cfg.TOKEN, self.cfg.DATA, augmentation)
        return SyntheticDrawings(int(self.cfg.get("SYNTHETIC_SAMPLES", n_default)), self._spec(), seed)

    def _split_on_disk(self, split_key):
        split = self.cfg.get(split_key)
        return bool(split) and all(os.path.exists(s) for s in str(split).split()) and os.path.isdir(str(self.cfg.get("ROOT", "")))

    def _device_loader(self, split_key, shuffle, drop_last, seed, augmentation):
        """``DEVICE_DATASET: true``: the split's drawings packed once into HBM and every batch tokenised there
        (device_data.py).  ``NUM_WORKERS`` has no meaning on this path."""
        from .device_data import DeviceDrawings, DeviceLoader, pack_infos
        dev = self.model._flat.device
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        cache = self.__dict__.setdefault("_device_drawings", {})       # a split is read and uploaded once, not per validation
        if (split_key, dev) not in cache:
            extract = {"auto": "auto", "true": True, "false": False}[self.extract_sideface] if self.device_kind == "sideface" else False
            render = {"auto": "auto", "true": True, "false": False}[self.render_drawings]
            # (pack_infos decides file by file, in its one pass: "auto" leaves a file that stores its input as it is)
            line = self.device_kind == "line"
            packed = pack_infos(str(self.cfg.get("ROOT", "")), parse_splits_list(self.cfg.get(split_key)), self.device_kind,
                                extract=extract, data_cfg=self.cfg.DATA if (extract or (line and render)) else None, render=render)
            cache[split_key, dev] = DeviceDrawings(packed, self.cfg.TOKEN, self.cfg.DATA, dev)
        return DeviceLoader(cache[split_key, dev], self.cfg.BATCH_SIZE, shuffle, drop_last, augmentation, seed)

    def _loader(self, split_key, n_default, shuffle, drop_last, seed, augmentation=False):
        if self.cfg.get("DEVICE_DATASET", False) and self._split_on_disk(split_key):
            return self._device_loader(split_key, shuffle, drop_last, seed, augmentation)
        ds = self._dataset(split_key, n_default, seed, augmentation)
        sampler = None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=shuffle, drop_last=drop_last)
            shuffle = False
        workers = int(self.cfg.get("NUM_WORKERS", 0)) if not isinstance(ds, SyntheticDrawings) else 0
        return torch.utils.data.DataLoader(ds, batch_size=self.cfg.BATCH_SIZE, shuffle=shuffle, drop_last=drop_last,
                                           num_workers=workers, sampler=sampler)

    def train_dataloader(self):
        return self._loader("DATASETS_TRAIN", 256, True, True, 2022, self.train_augmentation)

    def val_dataloader(self):
        return self._loader("DATASETS_VALID", 64, False, False, 9_000_000)

    def test_dataloader(self):
        return self._loader("DATASETS_TEST", 64, False, False, 9_500_000)

    # ------------------------------------------------------------------ steps
    def training_step(self, batch, batch_idx):
        st = self.seq_train
        if st is not None and self.global_step >= st["start_step"]:
            # sequence-level step: sample, score and re-weight on the device, then the usual train_step
            rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
            outputs = self.model.seq_train_step(batch, seed=seq_train_seed(st["seed"], self.global_step, rank),
                                                threshold=self.cfg.THRESHOLD, **st["step"])
            self._train_reward = outputs["reward"].detach()
        else:
            outputs = self.model(batch)
        loss = torch.mean(outputs["loss"])
        self._train_stats = (loss.detach(), torch.mean(outputs["accuracy"]).detach())
        # the plain mean NLL next to a smoothed / weighted loss (the model returns it only then; batch["loss_weight"] reaches it as is)
        self._train_nll = outputs["nll"].detach() if "nll" in outputs else None
        return loss

    def _valid_pred(self, pred):
        """reference trainer_complete.py:78-79 / 100-101: drop boxes with a zero extent (row 0 = bbox kept)."""
        if len(pred) <= 1:
            return pred
        ok = torch.all(torch.abs(pred[1:, 3:] - pred[1:, :3]) != 0, dim=1)
        return torch.concat((pred[:1], pred[1:][ok]))

    def _add_reprojection(self, batch, samples):
        """REPROJECTION_METRIC: the reprojection F1 of the returned programs joins the running sums; nothing is read back."""
        if not self.reprojection_metric:
            return
        f1 = self.model.reprojection(batch, samples)["reprojection_f1"]
        sums = torch.stack((f1.sum(), torch.full((), float(f1.numel()), dtype=torch.float64, device=f1.device)))
        self._reprojection_sums = sums if self._reprojection_sums is None else self._reprojection_sums + sums

    VOLUME_KEYS = ("volume_iou", "volume_precision", "volume_recall", "self_overlap")

    def _add_volume(self, batch, samples):
        """VOLUME_METRIC: the four volume scores of the returned programs join the running sums; nothing is read back."""
        if not self.volume_metric:
            return
        r = self.model.volume(batch, samples)
        n = r["volume_iou"].numel()
        sums = torch.stack([r[k].sum() for k in self.VOLUME_KEYS] + [torch.full((), float(n), dtype=torch.float64, device=r["volume_iou"].device)])
        self._volume_sums = sums if self._volume_sums is None else self._volume_sums + sums

    def validation_step(self, batch, batch_idx):
        if self.device_metric:
            outputs = self.model.eval_step(batch, parse=False)
            self.scorer.add_batch(outputs["samples"], batch["output_value"])
            self._add_reprojection(batch, outputs["samples"])
            self._add_volume(batch, outputs["samples"])
            return
        outputs = self.model(batch)
        for pred, gt in zip(outputs["predicts"], outputs["groundtruths"]):
            self.scorer.add(self._valid_pred(pred), gt)
        self._add_reprojection(batch, outputs["samples"])
        self._add_volume(batch, outputs["samples"])

    def _log_means(self, stage):
        for key, value in zip(("precision", "recall", "fmeasure"), self.scorer.means()):
            self.log(f"{stage}/{key}", value)
        if self.reprojection_metric:
            sums, self._reprojection_sums = self._reprojection_sums, None
            sums = allreduce_metric_sums(torch.zeros(2, dtype=torch.float64) if sums is None else sums.cpu())
            self.log(f"{stage}/reprojection_f1", float(sums[0]) / max(float(sums[1]), 1.0))
        if self.volume_metric:
            sums, self._volume_sums = self._volume_sums, None
            sums = allreduce_metric_sums(torch.zeros(5, dtype=torch.float64) if sums is None else sums.cpu())
            for i, key in enumerate(self.VOLUME_KEYS):
                self.log(f"{stage}/{key}", float(sums[i]) / max(float(sums[4]), 1.0))

    def validation_epoch_end(self, outputs=None):
        self._log_means("val")

    def _device_test_rows(self, batch, keep=None):
        """DEVICE_METRIC test_step: decode without the per-row parse, one matching launch, then per drawing (name, kept planks
        [n, 6], ground-truth planks, attach row, scores).  Beside the scorer's read-back of its integers, ONE device-to-host
        copy per batch: decoded tokens, attach and ground-truth tokens side by side in one tensor."""
        outputs = self.model.eval_step(batch, parse=False)
        self._add_reprojection(batch, outputs["samples"])
        self._add_volume(batch, outputs["samples"])
        scores = self.scorer.add_batch(outputs["samples"], batch["output_value"], scores=True, keep=keep)
        end = self.cfg.TOKEN.END
        n = outputs["samples"].shape[1]
        rows = torch.cat((outputs["samples"], outputs["attach"], batch["output_value"].to(outputs["samples"].device)), 1).cpu().numpy()
        samples, attach, truth = rows[:, :n], rows[:, n:2 * n], rows[:, 2 * n:]
        for i, name in enumerate(batch["name"]):
            yield name, valid_planks(planks_of_row(samples[i], end)), planks_of_row(truth[i], end), attach[i], scores[i]

    def test_step(self, batch, batch_idx):
        out_dir = os.path.join(self.logger.log_dir, "pred_jsons")
        os.makedirs(out_dir, exist_ok=True)
        if self.device_metric:
            for name, vp, gt, atta, scores in self._device_test_rows(batch):
                atta = atta[: vp.size]
                atta = atta[: len(atta) // 6 * 6].reshape(-1, 6).tolist()
                self._write_pred_json(out_dir, name, {"prediction": vp.reshape(-1, 6).tolist(), "attach": atta,
                                                      "groundtruth": gt.reshape(-1, 6).tolist(), **scores})
            return
        outputs = self.model(batch)
        self._add_reprojection(batch, outputs["samples"])
        self._add_volume(batch, outputs["samples"])
        for name, pred, gt, atta in zip(batch["name"], outputs["predicts"], outputs["groundtruths"], outputs["attach"]):
            vp = self._valid_pred(pred)
            scores = self.scorer.add(vp, gt)
            atta = atta[: vp.numel()].cpu().numpy()
            atta = atta[: len(atta) // 6 * 6].reshape(-1, 6).tolist()
            self._write_pred_json(out_dir, name, {"prediction": vp.cpu().numpy().reshape(-1, 6).tolist(), "attach": atta,
                                                  "groundtruth": gt.cpu().numpy().reshape(-1, 6).tolist(), **scores})

    @staticmethod
    def _write_pred_json(out_dir, name, record):
        """One `pred_jsons/<name>.json` in the reference's on-disk format (trainer_complete.py:104-118)."""
        with open(os.path.join(out_dir, f"{name}.json"), "w") as f:
            json.dump(record, f, indent=4, separators=(", ", ": "))

    def test_epoch_end(self, outputs=None):
        self._log_means("test")

    def configure_optimizers(self):
        from .optim import FusedAdam
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        return {"optimizer": FusedAdam(self.model, lr=self.cfg.LR, grad_scale=1.0 / world, **self.optimizer_kwargs,
                                       **self.recipe["optimizer"])}

    def scheduled_lr(self, base_lr, step, total_steps):
        """The learning rate of optimizer step ``step`` (0-based count of attempted steps = ``global_step``)."""
        from .optim import lr_factor
        sch = self.recipe["schedule"]
        total = sch["total_steps"] if sch["total_steps"] is not None else int(total_steps)
        return base_lr * lr_factor(sch["kind"], int(step), sch["warmup_steps"], total, sch["min_ratio"])

    # ------------------------------------------------------------------ checkpoints (Lightning-shaped)
    def checkpoint(self, epoch, optimizer=None, best_score=None, steps_this_epoch=0, best_path="", last_path="",
                   epoch_finished=True):
        """A pytorch_lightning-1.7-shaped checkpoint dict, the layout ModelCheckpoint writes for the reference
        (configs/train_complete.yaml:6-14): `state_dict` with the `model.` prefix, `optimizer_states` in
        torch.optim.Adam's layout, `hyper_parameters` (save_hyperparameters(hparams), trainer_complete.py:24), epoch /
        global_step, and the loop / callback records of `lightning_state`.  Guaranteed (tested) interop: weights +
        hyper-parameters + Adam state, both directions, and `fit --ckpt_path` resume inside THIS trainer.  The loop and
        callback records follow Lightning 1.7's schema from its source but no Lightning process has read them (it is
        not installable here), so resuming one of these files inside Lightning itself is unverified - INTEGRATION.md."""
        from . import lightning_state as LS
        ck = {"epoch": epoch, "global_step": self.global_step, "pytorch-lightning_version": "1.7.7",
              "state_dict": {"model." + k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
              "loops": LS.loops_state(epoch + 1, self.global_step, steps_this_epoch, epoch_finished=epoch_finished),
              "callbacks": {LS.checkpoint_callback_key(): LS.checkpoint_callback_state(best_score, best_path, last_path,
                                                                                       os.path.dirname(last_path))},
              "optimizer_states": [], "lr_schedulers": [],
              "hparams_name": "hparams", "hyper_parameters": {"hparams": self.hparams_dict}}
        if optimizer is not None:
            ck["optimizer_states"] = [optimizer.torch_state_dict() if hasattr(optimizer, "torch_state_dict")
                                      else optimizer.state_dict()]
            ema = optimizer.ema_state_dict() if hasattr(optimizer, "ema_state_dict") else None
            if ema is not None:                # the raw weights stay in `state_dict` (exact resume); the EMA travels beside them
                ck["ema_state_dict"] = {"model." + k: v for k, v in ema.items()}
                ck["ema_updates"] = int(optimizer.ema_updates)
            if self.recipe["schedule"]["kind"] != "constant" and hasattr(optimizer, "base_lr"):
                # one record in the shape of torch.optim.lr_scheduler.LambdaLR.state_dict(); _last_lr: the rate of the NEXT step
                total = getattr(self, "lr_total_steps", 0)
                ck["lr_schedulers"] = [{"last_epoch": self.global_step, "_step_count": self.global_step + 1,
                                        "base_lrs": [optimizer.base_lr],
                                        "_last_lr": [self.scheduled_lr(optimizer.base_lr, self.global_step, total)]}]
        return ck

    @staticmethod
    def _read_checkpoint_file(path):
        """torch.load restricted to tensors / containers / plain scalars (`weights_only=True`).  A file that needs more
        than that (arbitrary pickled objects - older Lightning files can carry argparse Namespaces or callback objects) is
        refused unless PLANK_TRUST_CHECKPOINT=1: unpickling runs code from the file, and `--ckpt_path` is user input."""
        import pickle
        try:
            return torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as exc:
            if os.environ.get("PLANK_TRUST_CHECKPOINT") != "1":
                raise RuntimeError(f"{path}: not loadable with weights_only=True ({exc}); set PLANK_TRUST_CHECKPOINT=1 to "
                                   f"unpickle it anyway - only for files you trust") from exc
            print(f"[plankassembly_amd] WARNING: unpickling {path} without restrictions (PLANK_TRUST_CHECKPOINT=1)")
            return torch.load(path, map_location="cpu", weights_only=False)

    def load_checkpoint(self, path, optimizer=None, use_ema=False):
        """Weights always; with ``optimizer`` also the Adam moments / step, the EMA, the schedule record, epoch and global_step
        (what Lightning's ``fit --ckpt_path`` resumes).  ``use_ema`` (without ``optimizer``): the weights loaded are the file's
        ``ema_state_dict`` when it has one.  Returns the checkpoint dict."""
        from . import lightning_state as LS
        ck = self._read_checkpoint_file(path)
        sd = ck.get("state_dict", ck)
        if optimizer is None and use_ema and ck.get("ema_state_dict"):
            sd = ck["ema_state_dict"]
        strip = lambda d: {(k[6:] if k.startswith("model.") else k): v for k, v in d.items()}
        self.model.load_state_dict(strip(sd))
        if optimizer is not None and ck.get("optimizer_states"):
            optimizer.load_state_dict(ck["optimizer_states"][0])
        if optimizer is not None and ck.get("ema_state_dict") and getattr(optimizer, "ema_decay", None) is not None:
            optimizer.load_ema_state_dict(strip(ck["ema_state_dict"]), int(ck.get("ema_updates", 0)))
        if optimizer is not None and ck.get("lr_schedulers") and hasattr(optimizer, "base_lr"):
            rec = ck["lr_schedulers"][0]
            optimizer.base_lr = float(rec["base_lrs"][0])
            optimizer.param_groups[0]["lr"] = float(rec["_last_lr"][0])
        if optimizer is not None:
            self.global_step = int(ck.get("global_step", 0))
            self.resume_epoch = LS.epochs_done_of(ck)
            for key, state in (ck.get("callbacks") or {}).items():
                if str(key).startswith("ModelCheckpoint") and isinstance(state, dict) and state.get("best_model_score") is not None:
                    self.resume_best = float(state["best_model_score"])
                    # ModelCheckpoint restores best_model_path too: the file a better epoch must replace (save_top_k: 1)
                    self.resume_best_path = str(state.get("best_model_path") or "")
        return ck


class VisibleTrainer(Trainer):
    """reference trainer_visible.py: no augmentation in the train loader."""
    default_lines = (8, 249)
    train_augmentation = False


class SidefaceTrainer(Trainer):
    """reference trainer_sideface.py: side-face tokens, no ``input_type``; a sample with no detected
    side faces (input = [END, PAD...]) scores 0 and writes an empty prediction (:46-52)."""
    with_type = False
    default_lines = (0, 74)
    dataset_cls = SidefaceDataset
    device_kind = "sideface"

    def test_step(self, batch, batch_idx):
        out_dir = os.path.join(self.logger.log_dir, "pred_jsons")
        os.makedirs(out_dir, exist_ok=True)
        if self.device_metric:
            empty = torch.all(batch["input_mask"][:, 1:], dim=1).cpu().tolist()
            rows = self._device_test_rows(batch, keep=[not e for e in empty])
            for (name, vp, gt, _, scores), e in zip(rows, empty):
                predl = [] if e else vp.reshape(-1, 6).tolist()
                scores = {"precision": 0.0, "recall": 0.0, "fmeasure": 0.0} if e else scores
                self._write_pred_json(out_dir, name, {"prediction": predl, "groundtruth": gt.reshape(-1, 6).tolist(), **scores})
            return
        outputs = self.model(batch)
        for name, mask, pred, gt in zip(batch["name"], batch["input_mask"], outputs["predicts"], outputs["groundtruths"]):
            gtl = gt.cpu().numpy().reshape(-1, 6).tolist()
            if bool(torch.all(mask[1:])):
                predl, scores = [], {"precision": 0.0, "recall": 0.0, "fmeasure": 0.0}
            else:
                vp = self._valid_pred(pred)
                scores = self.scorer.add(vp, gt)
                predl = vp.cpu().numpy().reshape(-1, 6).tolist()
            self._write_pred_json(out_dir, name, {"prediction": predl, "groundtruth": gtl, **scores})


# ====================================================================================== loop + CLI
def _to_device(batch, dev, model=None):
    if model is not None and hasattr(model, "prepare_batch"):
        return model.prepare_batch(batch)
    return {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _flag(tkw, key):
    v = tkw.get(key)
    if v is None or isinstance(v, bool):
        return bool(v)
    if isinstance(v, str) and v.lower() in ("true", "false"):      # `--trainer.detect_anomaly True` arrives as a string
        return v.lower() == "true"
    raise ValueError(f"trainer.{key} must be a bool, got {v!r}")


def optimizer_options(tkw):
    """The gradient-guard keys of the `trainer:` block -> (FusedAdam keyword arguments, raise_on_skip).

    ``gradient_clip_val`` (None / 0: off) with ``gradient_clip_algorithm`` ``norm`` (default) or ``value``: Lightning's own
    keys, clip_grad_norm_ resp. clip_grad_value_ before the optimizer step.  ``detect_anomaly`` (the reference sets it,
    configs/train_complete.yaml:16 there: a run dies on a non-finite gradient): a step with a non-finite gradient is not
    applied, and the loop raises at the next epoch boundary - with the weights still clean.  ``skip_nonfinite_steps`` (this
    repository's key): the same skip without the raise."""
    kw = {}
    algo = tkw.get("gradient_clip_algorithm")
    algo = "norm" if algo is None else algo
    if algo not in ("norm", "value"):
        raise ValueError(f"trainer.gradient_clip_algorithm must be 'norm' or 'value', got {algo!r}")
    val = tkw.get("gradient_clip_val")
    if val is not None:
        if isinstance(val, bool) or not isinstance(val, (int, float)) or val != val or val < 0 or val == float("inf"):
            raise ValueError(f"trainer.gradient_clip_val must be a finite number >= 0 (0 / null: off), got {val!r}")
        if val > 0:
            kw["max_grad_norm" if algo == "norm" else "clip_value"] = float(val)
    raise_on_skip = _flag(tkw, "detect_anomaly")
    if raise_on_skip or _flag(tkw, "skip_nonfinite_steps"):
        kw["skip_nonfinite"] = True
    return kw, raise_on_skip


def _number(key, v, lo, hi, hi_open=False):
    ok = not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and lo <= v and (v < hi if hi_open else v <= hi)
    if not ok:
        raise ValueError(f"{key} must be a number in [{lo}, {hi}{')' if hi_open else ']'}, got {v!r}")
    return float(v)


def _count(key, v, lo=0):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{key} must be an integer >= {lo}, got {v!r}")
    return v


def _bool(key, v):
    if not isinstance(v, bool):
        raise ValueError(f"{key} must be a bool, got {v!r}")
    return v


def recipe_options(hparams):
    """The training-recipe keys of the hparams (next to ``LR``), validated -> {"optimizer": FusedAdam keyword arguments,
    "schedule": {kind, warmup_steps, total_steps, min_ratio}, "eval_ema": bool}.  All off by default.

    ``WEIGHT_DECAY`` (0) with ``NO_DECAY`` ``1d`` (default: biases and LayerNorm parameters do not decay) or ``none``;
    ``LR_SCHEDULE`` ``constant`` (default) / ``warmup`` / ``cosine`` / ``inverse_sqrt`` with ``WARMUP_STEPS`` (0), ``LR_TOTAL_STEPS``
    (null: the run's own length - max_steps, else max_epochs * batches per epoch) and ``MIN_LR_RATIO`` (0), see optim.lr_factor;
    ``EMA_DECAY`` (null: off) with ``EMA_WARMUP`` (false); ``EVAL_EMA`` (default: true exactly when EMA_DECAY is set): validation,
    and with it the best-checkpoint choice, and ``test --ckpt_path`` use the averaged weights."""
    from .optim import LR_SCHEDULES, NO_DECAY_MODES, lr_factor
    get = lambda k, d=None: d if hparams.get(k) is None else hparams.get(k)
    wd = _number("WEIGHT_DECAY", get("WEIGHT_DECAY", 0.0), 0.0, float("inf"), hi_open=True)
    no_decay = get("NO_DECAY", "1d")
    if no_decay not in NO_DECAY_MODES:
        raise ValueError(f"NO_DECAY must be one of {NO_DECAY_MODES}, got {no_decay!r}")
    kind = get("LR_SCHEDULE", "constant")
    if kind not in LR_SCHEDULES:
        raise ValueError(f"LR_SCHEDULE must be one of {LR_SCHEDULES}, got {kind!r}")
    warmup = _count("WARMUP_STEPS", get("WARMUP_STEPS", 0))
    total = hparams.get("LR_TOTAL_STEPS")
    if total is not None:
        total = _count("LR_TOTAL_STEPS", total, 1)
    min_ratio = _number("MIN_LR_RATIO", get("MIN_LR_RATIO", 0.0), 0.0, 1.0)
    lr_factor(kind, 0, warmup, total if total is not None else warmup + 1, min_ratio)     # (the schedule's own argument rules)
    ema = hparams.get("EMA_DECAY")
    if ema is not None:
        ema = _number("EMA_DECAY", ema, 0.0, 1.0, hi_open=True)
    ema_warmup = _bool("EMA_WARMUP", get("EMA_WARMUP", False))
    eval_ema = _bool("EVAL_EMA", get("EVAL_EMA", ema is not None))
    if eval_ema and ema is None:
        raise ValueError("EVAL_EMA: true needs EMA_DECAY")
    return {"optimizer": {"weight_decay": wd, "no_decay": no_decay, "ema_decay": ema, "ema_warmup": ema_warmup},
            "schedule": {"kind": kind, "warmup_steps": warmup, "total_steps": total, "min_ratio": min_ratio},
            "eval_ema": eval_ema}


SEQ_TRAIN_KEYS = ("NUM_SAMPLES", "TEMPERATURE", "TOP_K", "TOP_P", "OBJECTIVE", "BASELINE", "ALPHA", "NLL_WEIGHT", "CONSTRAIN_PLANKS",
                  "START_STEP", "SEED", "SHARE_ENCODER")


def seq_train_options(hparams):
    """The optional ``SEQ_TRAIN`` block of the hparams (sequence-level training on plank F1), validated ->
    None when the block is absent (the feature is off), else {"step": PlankModel.seq_train_step keyword arguments without the
    seed, "start_step": int, "seed": int}.  Every bad value raises a ValueError that names its key.

    ``NUM_SAMPLES`` (required, 1 .. 64), ``TEMPERATURE`` (1), ``TOP_K`` (0 = off), ``TOP_P`` (1 = off): the sampling;
    ``OBJECTIVE`` ``reinforce`` (default) / ``risk`` with ``BASELINE`` ``none`` / ``mean`` (default; NUM_SAMPLES >= 2) / ``greedy``
    and ``ALPHA`` (1; > 0, the sharpness of the risk's softmax); ``NLL_WEIGHT`` (0): the weight of each drawing's ground-truth row,
    0 = no such row; ``CONSTRAIN_PLANKS`` (null: the model's own MODEL.CONSTRAIN_PLANKS; true: the default grammar; false: none);
    ``START_STEP`` (0): the first global step trained this way, the steps before it are plain NLL steps; ``SEED`` (0): see
    ``seq_train_seed``; ``SHARE_ENCODER`` (null: the model's own MODEL.SHARE_ENCODER; a bool: the step's ``share_encoder``, DESIGN.md
    section 25 - the key is in "step" only when the block sets it)."""
    from .decode import sample_params
    from .ops import SEQ_BASELINES, SEQ_OBJECTIVES
    blk = hparams.get("SEQ_TRAIN")
    if blk is None:
        return None
    if not isinstance(blk, dict):
        raise ValueError(f"SEQ_TRAIN must be a mapping of {SEQ_TRAIN_KEYS}, got {blk!r}")
    unknown = sorted(set(blk) - set(SEQ_TRAIN_KEYS))
    if unknown:
        raise ValueError(f"SEQ_TRAIN has unknown key(s) {unknown}; known: {SEQ_TRAIN_KEYS}")
    get = lambda k, d=None: d if blk.get(k) is None else blk.get(k)
    if blk.get("NUM_SAMPLES") is None:
        raise ValueError("SEQ_TRAIN needs NUM_SAMPLES (an integer in [1, 64])")
    n, temp, top_k, top_p = blk["NUM_SAMPLES"], get("TEMPERATURE", 1.0), get("TOP_K", 0), get("TOP_P", 1.0)
    sample_params(n, temp, top_k, top_p, 0)                        # ValueError naming NUM_SAMPLES / TEMPERATURE / TOP_K / TOP_P
    seed = get("SEED", 0)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"SEED must be an integer in [0, 2^32), got {seed!r}")
    objective = get("OBJECTIVE", "reinforce")
    if objective not in SEQ_OBJECTIVES:
        raise ValueError(f"OBJECTIVE must be one of {SEQ_OBJECTIVES}, got {objective!r}")
    baseline = get("BASELINE", "mean")
    if baseline not in SEQ_BASELINES:
        raise ValueError(f"BASELINE must be one of {SEQ_BASELINES}, got {baseline!r}")
    if baseline == "mean" and n < 2:
        raise ValueError(f"BASELINE 'mean' needs NUM_SAMPLES >= 2, got {n!r}")
    alpha = _number("ALPHA", get("ALPHA", 1.0), 0.0, float("inf"), hi_open=True)
    if alpha <= 0.0:
        raise ValueError(f"ALPHA must be a number > 0, got {alpha!r}")
    nll_weight = _number("NLL_WEIGHT", get("NLL_WEIGHT", 0.0), float("-inf"), float("inf"), hi_open=True)
    if nll_weight == float("-inf"):
        raise ValueError(f"NLL_WEIGHT must be a finite number, got {nll_weight!r}")
    constrain = blk.get("CONSTRAIN_PLANKS")
    if constrain is not None:
        constrain = _bool("CONSTRAIN_PLANKS", constrain)
    start = _count("START_STEP", get("START_STEP", 0))
    step = {"num_samples": n, "temperature": float(temp), "top_k": top_k, "top_p": float(top_p), "objective": objective,
            "baseline": baseline, "alpha": alpha, "nll_weight": nll_weight, "constraint": constrain}
    if blk.get("SHARE_ENCODER") is not None:
        step["share_encoder"] = _bool("SHARE_ENCODER", blk["SHARE_ENCODER"])
    return {"step": step, "start_step": start, "seed": seed}


def extract_option(hparams):
    """``DATA.EXTRACT_SIDEFACE`` of the hparams, validated -> ``auto`` (default: side faces are extracted from the line drawing
    where the info files store none), ``true`` (always extracted from ``svgs`` - what train-time augmentation needs) or ``false``
    (stored ``faces`` only).  Read by the sideface kind's CPU dataset and device dataset alike."""
    data = hparams.get("DATA") or {}
    return extract_mode(data.get("EXTRACT_SIDEFACE") if hasattr(data, "get") else None)


def render_option(hparams):
    """``DATA.RENDER_DRAWINGS`` of the hparams, validated -> ``auto`` (default: the drawing is rendered from the planks where the
    info files store none), ``true`` (always rendered) or ``false`` (stored lines only).  Read by the CPU datasets and the line
    kind's device dataset alike."""
    data = hparams.get("DATA") or {}
    return render_mode(data.get("RENDER_DRAWINGS") if hasattr(data, "get") else None)


def reprojection_option(hparams, device_kind="line", num_output_dof=6):
    """``REPROJECTION_METRIC`` of the hparams, validated -> bool (default False): validation and test also log
    ``val/reprojection_f1`` / ``test/reprojection_f1``, the mean reprojection F1 of the returned programs (DESIGN.md section 30;
    its tolerance and type mode are MODEL.REPROJECTION_TOL / REPROJECTION_TYPES).  The score is defined for line drawings and
    planks of six DOF: the sideface kind and any other DOF are refused."""
    v = hparams.get("REPROJECTION_METRIC")
    if v is None:
        return False
    if not isinstance(v, bool):
        raise ValueError(f"REPROJECTION_METRIC must be a bool, got {v!r}")
    if v and device_kind != "line":
        raise ValueError("REPROJECTION_METRIC compares line drawings: the tokens of a sideface input are faces, not lines")
    if v and int(num_output_dof) != 6:
        raise ValueError("REPROJECTION_METRIC renders planks of six output DOF")
    return v


def volume_option(hparams, num_output_dof=6):
    """``VOLUME_METRIC`` of the hparams, validated -> bool (default False): validation and test also log ``val/`` and ``test/``
    ``volume_iou`` / ``volume_precision`` / ``volume_recall`` / ``self_overlap``, the means over drawings of the returned programs
    as solids against their ground truth.  Any input kind; planks of six DOF only."""
    v = hparams.get("VOLUME_METRIC")
    if v is None:
        return False
    if not isinstance(v, bool):
        raise ValueError(f"VOLUME_METRIC must be a bool, got {v!r}")
    if v and int(num_output_dof) != 6:
        raise ValueError("VOLUME_METRIC compares planks of six output DOF")
    return v


def seq_train_seed(seed, global_step, rank):
    """The sampling seed of a sequence-level training step: (SEED + 4096 * global_step + rank) mod 2^32 - a pure function of its
    arguments, so a resumed run draws what the uninterrupted one would have drawn; distinct for every (step, rank) with rank < 4096
    within any 2^20 consecutive steps.  (The sampler hashes the seed - pa_decode_sample_begin - so neighbouring seeds share nothing.)"""
    return (int(seed) + 4096 * int(global_step) + int(rank)) % 2 ** 32


def ema_checkpoint(ck):
    """A copy of checkpoint dict ``ck`` whose ``state_dict`` is the EMA: the file to hand to the reference, which knows no
    ``ema_state_dict`` key.  The raw weights are dropped from the copy, so it is for evaluation, not for an exact resume."""
    if "ema_state_dict" not in ck:
        raise KeyError("ema_checkpoint(): the checkpoint has no ema_state_dict (written with EMA_DECAY set)")
    out = {k: v for k, v in ck.items() if k not in ("ema_state_dict", "ema_updates")}
    out["state_dict"] = {k: v.clone() for k, v in ck["ema_state_dict"].items()}
    return out


def run(trainer_cls, subcommand, config, ckpt_path=None, overrides=None):
    """The part of ``pl.Trainer.fit/test`` the reference relies on."""
    seed, tkw, hparams = load_cli_config(config)
    for k, v in (overrides or {}).items():
        tkw[k] = v
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # PLANK_DIST_BACKEND=gloo is for TESTS (tests/test_cli_gpu.py): RCCL refuses two ranks on one device; with gloo the ranks of a
    # one-GPU box share cuda:0 and the whole DDP path of this loop (DistributedSampler shards, GradSync, metric sums) still runs.
    backend = os.environ.get("PLANK_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local %= torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    if seed is not None:
        torch.manual_seed(int(seed)); np.random.seed(int(seed))
    module = trainer_cls(hparams)
    module.logger = _Logger()
    if world > 1:                                  # one lightning_logs/version_N for the whole job: rank 0's choice
        box = [module.logger.log_dir]
        dist.broadcast_object_list(box, src=0)
        module.logger.log_dir = box[0]
    dev = torch.device("cuda", local)
    module.model.to(dev)
    if ckpt_path and subcommand == "test":
        module.load_checkpoint(ckpt_path, use_ema=module.recipe["eval_ema"])
    if subcommand == "test":
        module.model.eval()
        with torch.no_grad():
            for i, batch in enumerate(module.test_dataloader()):
                module.test_step(_to_device(batch, dev, module.model), i)
        module.test_epoch_end()
        if rank == 0:
            print({k: round(v, 4) for k, v in module._logged.items()})
        return module
    module.optimizer_kwargs, raise_on_skip = optimizer_options(tkw)
    opt = module.configure_optimizers()["optimizer"]
    module.optimizer = opt
    start_epoch, best, best_file = 0, -1.0, ""
    if ckpt_path:                                  # fit --ckpt_path: weights + Adam state + counters, like Lightning
        module.load_checkpoint(ckpt_path, optimizer=opt)
        start_epoch = getattr(module, "resume_epoch", 0)
        best = getattr(module, "resume_best", -1.0)
        best_file = getattr(module, "resume_best_path", "")
        if best_file and not os.path.exists(best_file):
            best_file = ""
    guard_base = module.global_step                # the guard counts attempts from here (optimizer built / state loaded)
    sync = None
    if world > 1:
        from .distributed import GradSync
        sync = GradSync(module.model)
        sync.broadcast_parameters(0)
    max_epochs = int(tkw.get("max_epochs", 1))
    every = int(tkw.get("check_val_every_n_epoch", 1))
    max_steps = int(tkw.get("max_steps", -1))
    loader = module.train_dataloader()
    scheduled = module.recipe["schedule"]["kind"] != "constant"
    module.lr_total_steps = max_steps if max_steps > 0 else max_epochs * (len(loader) if hasattr(loader, "__len__") else 0)
    eval_weights = opt.ema_weights if module.recipe["eval_ema"] else contextlib.nullcontext
    for epoch in range(start_epoch, max_epochs):
        if 0 < max_steps <= module.global_step:            # a resumed run whose epoch was cut by max_steps: nothing left to do
            break
        module.model.train()
        if hasattr(loader, "set_epoch"):                   # device_data.DeviceLoader: sampler order and augmentation draws
            loader.set_epoch(epoch)
        elif hasattr(loader.sampler, "set_epoch"):
            loader.sampler.set_epoch(epoch)
        t0, n, steps_here = time.perf_counter(), 0, 0
        from .data import DevicePrefetcher
        n_batches = len(loader) if hasattr(loader, "__len__") else -1
        for i, batch in enumerate(DevicePrefetcher(module.model, loader)):     # batch i + 1 is prepared while step i runs
            opt.zero_grad()
            loss = module.training_step(batch, i)
            loss.backward()
            if scheduled:                                  # keyed on the steps attempted so far: host-known, no read-back
                opt.param_groups[0]["lr"] = module.scheduled_lr(opt.base_lr, module.global_step, module.lr_total_steps)
            opt.step()
            module.global_step += 1
            steps_here += 1
            n += batch["input_value"].shape[0]
            if 0 < max_steps <= module.global_step:
                break
        l, a = module._train_stats
        module.log("train/loss", l); module.log("train/accuracy", a)
        if getattr(module, "_train_nll", None) is not None:
            module.log("train/nll", module._train_nll)
        if getattr(module, "_train_reward", None) is not None:     # mean sample F1 of the epoch's last sequence-level step
            module.log("train/reward", module._train_reward)
        module.log("train/lr", opt.param_groups[0]["lr"])      # the rate of the epoch's last step
        torch.cuda.synchronize()
        if getattr(opt, "guarded", False):                 # the guard's one read-back, where the loop synchronises anyway
            gs = opt.guard_stats()
            module.log("train/grad_norm", gs["norm"]); module.log("train/skipped_steps", gs["skipped_steps"])
            if raise_on_skip and gs["skipped_steps"] > 0:
                # every rank sees the same summed gradients, so every rank skipped the same steps and raises here
                raise RuntimeError(
                    f"detect_anomaly: {gs['skipped_steps']} optimizer step(s) had a non-finite gradient and were not applied; "
                    f"the first at global step {guard_base + gs['first_skipped_attempt'] - 1} (epoch {epoch}). The weights "
                    f"hold only the steps with finite gradients.")
        if rank == 0:
            print(f"epoch {epoch}: train/loss {float(l):.4f} train/accuracy {float(a):.4f} "
                  f"{n * world / (time.perf_counter() - t0):.1f} samples/s")
        finished = not (0 <= steps_here < n_batches)       # False: max_steps cut the epoch short - a resume runs it again
        if (epoch + 1) % every == 0:
            ckdir = os.path.join(module.logger.log_dir, "checkpoints")
            last = os.path.join(ckdir, "last.ckpt")
            if rank == 0:                                              # save_last: before the metric exchange, so a failure
                os.makedirs(ckdir, exist_ok=True)                      # in validation cannot lose the epoch's weights
                torch.save(module.checkpoint(epoch, opt, best if best >= 0 else None, steps_here, best_file, last,
                                             epoch_finished=finished), last)
            module.model.eval()
            with torch.no_grad(), eval_weights():
                for i, batch in enumerate(module.val_dataloader()):
                    module.validation_step(_to_device(batch, dev, module.model), i)
            module.validation_epoch_end()
            f1 = module._logged.get("val/fmeasure", 0.0)
            if rank == 0:
                improved = f1 > best                                   # ModelCheckpoint(monitor=val/fmeasure, mode=max)
                if improved:
                    best = f1
                    stale, best_file = best_file, os.path.join(ckdir, (
                        f"checkpoint_{epoch:03d}-precision={module._logged['val/precision']:.3f}-"
                        f"recall={module._logged['val/recall']:.3f}-f1={f1:.3f}.ckpt"))
                ck = module.checkpoint(epoch, opt, best, steps_here, best_file, last, epoch_finished=finished)
                torch.save(ck, last)
                if improved:
                    torch.save(ck, best_file)
                    # save_top_k: 1 - but only among THIS run's checkpoints.  A best file inherited from the checkpoint being
                    # resumed lives in an earlier run's version_N/checkpoints (often it IS --ckpt_path): Lightning 1.7 restores
                    # best_model_path only for a matching dirpath and never deletes another run's file; neither do we.
                    if (stale and stale != best_file and os.path.exists(stale)
                            and os.path.abspath(os.path.dirname(stale)) == os.path.abspath(ckdir)
                            and not (ckpt_path and os.path.abspath(stale) == os.path.abspath(ckpt_path))):
                        os.remove(stale)
                print({k: round(v, 4) for k, v in module._logged.items() if k.startswith("val/")})
        if 0 < max_steps <= module.global_step:
            break
    if sync is not None:
        dist.barrier()
    return module


def cli(trainer_cls, argv=None):
    """``python trainer_complete.py fit --config configs/train_complete.yaml [--ckpt_path x] [--trainer.devices 1]``"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in ("fit", "test", "validate"):
        raise SystemExit("usage: <trainer>.py {fit,test} --config CONFIG [--ckpt_path CKPT] [--trainer.KEY VALUE ...]")
    sub, config, ckpt, over = argv[0], None, None, {}
    i = 1
    while i < len(argv):
        key, val = argv[i], argv[i + 1] if i + 1 < len(argv) else None
        if "=" in key:
            key, val = key.split("=", 1)
            i += 1
        else:
            i += 2
        if key == "--config":
            config = val
        elif key == "--ckpt_path":
            ckpt = val
        elif key.startswith("--trainer."):
            try:
                val = json.loads(val)
            except (ValueError, TypeError):
                pass
            over[key[len("--trainer."):]] = val
        else:
            raise SystemExit(f"unknown argument {key}")
    if config is None:
        raise SystemExit("--config is required")
    return run(trainer_cls, "test" if sub != "fit" else "fit", config, ckpt, over)
