"""``experiments.bpr.Experiment`` — what the reference's BPR configs instantiate
(experiments/bpr/exp.py:44-405 of the reference), reduced to the training path: build model /
optimizer / loaders from the config, wire negative sampling, seen-item masking, metrics, early
stopping and per-epoch logging onto the two-engine ``Trainer``, run.  Trackers (W&B / ClearML),
accelerate checkpoints, S3 and Optuna are out of scope; the constructor
still accepts their arguments so configs load unchanged.

Negative sampling runs on the device: the training dataset's seen-items CSR is bound to the engine
once, and the per-batch handler calls the device samplers (uniform when
``adaptive_sampling_prob`` is unset — exp.py:356-367 of the reference).
"""
from __future__ import annotations

import json
import logging
import math
import random
import time
from pathlib import Path
from typing import Any, Callable, Literal, Optional

import numpy as np
import torch

from experiments.config import instantiate
from experiments.trainer import Events, ModelEvents, NullAccelerator, Trainer
from revisit_bpr.modules import AdaptiveSampler, UniformSampler

log = logging.getLogger("experiments.bpr")


def _seed_worker(worker_id: int) -> None:
    seed = torch.initial_seed() % 2 ** 32
    np.random.seed(seed)
    random.seed(seed)


class BPRExperiment:
    def __init__(self, exp_config, dir: Optional[Path] = None, n_checkpoints: int = 2,
                 mixed_precision: Optional[str] = None, datasets_key: str = "datasets",
                 metrics: Optional[dict] = None, trackers_params: Optional[dict] = None,
                 events: Optional[dict] = None, seed: int = 13, debug: bool = False,
                 skip_seen: bool = True, save_logits: bool = False,
                 save_user_metrics: bool = False, log_momentum: bool = False,
                 early_stopping_metric: Optional[str] = None, early_stopping_patience: int = 200,
                 early_stopping_direction: Literal["min", "max"] = "max",
                 neg_sampling_alpha: float = 0.0,
                 adaptive_sampling_prob: Optional[float] = None,
                 train_mode: Literal["auto", "api", "strict", "stream"] = "auto") -> None:
        self._config = exp_config if isinstance(exp_config, dict) else exp_config()
        self._dir = Path(dir) if dir is not None else None
        self._datasets_key = datasets_key
        self._metrics = metrics or {}
        self._events = events or {}
        self._seed = seed
        self._debug = debug
        self._skip_seen = skip_seen
        self._early = (early_stopping_metric, early_stopping_patience, early_stopping_direction)
        self._adaptive_p = adaptive_sampling_prob
        if train_mode not in ("auto", "api", "strict", "stream"):
            raise ValueError("train_mode must be 'auto', 'api', 'strict' or 'stream'")
        # "api": the reference's per-batch loop (DataLoader -> sampler -> model -> backward -> step):
        #        ~170 us of interpreter per batch, 1.5 M triples/s whatever the kernels do;
        # "strict": the same mini-batches, whole epochs inside the library (any optimizer): 5-12 M;
        # "stream": the fused throughput paths (plain SGD: the STREAM kernel; Adam / momentum /
        # RMSprop: the batched STREAM kernel).  Extension: the reference has only the first.
        # "auto" (default, r5): "strict" when nothing can tell the difference — the fused model on a
        # ROCm device, the in-memory sparse dataset behind a shuffling DataLoader, no user handlers on
        # the train engine, not the debug run (its every-2000-iterations cut) — else "api".  An
        # unchanged config then trains at the library's rate instead of the interpreter's.
        self._train_mode = train_mode
        # item weights of the static sampler: count ** neg_sampling_alpha for the items listed in the
        # datasets' `item_counts` file, 1 elsewhere (reference: exp.py:85-91)
        self._item_counts = None
        path = self._config.get(datasets_key, {}).pop("item_counts", None) \
            if isinstance(self._config.get(datasets_key), dict) else None
        if path is not None:
            counts = torch.ones(self._config["num_items"], dtype=torch.float32)
            with open(path, "r", encoding="utf-8") as file:
                for rec in map(json.loads, file):
                    counts[rec["item"]] = float(rec["count"]) ** neg_sampling_alpha
            self._item_counts = counts
        self._state = None
        self._eval_fused = False
        self.history: list[dict] = []

    @property
    def metrics(self) -> dict[str, Any]:
        return self._state.metrics if self._state is not None else {}

    # ---- setup ------------------------------------------------------------------------------
    def _seed_everything(self) -> None:
        random.seed(self._seed)
        np.random.seed(self._seed)
        torch.manual_seed(self._seed)

    def run(self) -> Any:
        cfg = self._config
        self._accelerator = acc = NullAccelerator()
        self._seed_everything()
        self._model = instantiate(cfg["model"]).to(acc.device)
        self._optimizer = instantiate(cfg["optimizer"])(self._model.parameters())
        dcfg = cfg[self._datasets_key]
        max_iters = {k: d.pop("max_iters", None) for k, d in dcfg.items() if isinstance(d, dict)}
        self._datasets = {}
        for key, loader_cfg in dcfg.items():
            loader = instantiate(loader_cfg, generator=torch.Generator().manual_seed(self._seed),
                                 worker_init_fn=_seed_worker)
            if hasattr(loader.dataset, "collate_fn"):
                loader.collate_fn = loader.dataset.collate_fn
            self._datasets[key] = loader
        for m in self._metrics.values():
            m.set_accelerator(acc)
        train_ds = self._datasets["train"].dataset
        if hasattr(train_ds, "seen_csr") and hasattr(self._model, "bind_seen_csr"):
            indptr, indices = train_ds.seen_csr()
            self._model.bind_seen_csr(indptr.to(acc.device), indices.to(acc.device))
        num_items = cfg["num_items"]
        if self._item_counts is not None and hasattr(self._model, "engine"):
            self._model.engine().bind_item_weights(self._item_counts)  # strict / stream epochs
        if isinstance(self._adaptive_p, float):
            # the refresh is driven by the GET_BATCH_COMPLETED(every=...) handler below, which
            # runs BEFORE the sampling handler, as in the reference (exp.py:197-208)
            self._sampler = AdaptiveSampler(self._model, num_items, self._adaptive_p,
                                            None, every=10 ** 18)
        else:
            self._sampler = UniformSampler(num_items, None, item_weights=self._item_counts)
        if self._train_mode == "auto":
            self._train_mode = self._pick_train_mode()
        self.trainer = self._build_trainer()
        # "In case of preemptible tasks neg generator might sample the same data" (reference
        # exp.py:124-128): the generator is seeded with seed + the train engine's iteration, which
        # is where a resumed run continues (0 on a fresh start)
        self._neg_gen = torch.Generator(device=acc.device).manual_seed(
            self._seed + int(getattr(self.trainer.engines["train"].state, "iteration", 0) or 0))
        self._sampler._neg_gen = self._neg_gen
        loaders = self._datasets
        if self._train_mode != "api":
            loaders = self._install_fast_epochs(max_iters)
            if self._can_fuse_eval(max_iters):
                loaders = self._install_fast_eval(loaders)
        elif isinstance(self._adaptive_p, float):
            self._sampler.update_stats()
        self._state = self.trainer.run(loaders, max_iters=max_iters, epochs=cfg["epochs"])
        if self._dir is not None:
            self._dir.mkdir(parents=True, exist_ok=True)
            (self._dir / "history.json").write_text(json.dumps(self.history, indent=1))
        return self._state

    def _pick_train_mode(self) -> str:
        """`auto`: whole epochs inside the library when nothing can tell the difference — the fused model on a ROCm
        device, the in-memory sparse dataset behind a plain shuffling DataLoader (default batch sampler, no
        drop_last), no custom engines, no user handlers on the train engine, not the debug run — and then
          "stream"  for plain SGD while the launch is inside the staleness budget (`fast.lag_within_budget`: the rule
                    tests/test_gpu_fullscale_reference.py pins to the reference's own loop and to exact mini-batches),
          "strict"  otherwise (the reference's mini-batches, any optimizer, any learning rate);
        else "api", the reference's per-batch loop.  The choice is logged."""
        from torch.utils.data import BatchSampler, RandomSampler

        loader = self._datasets.get("train")
        ds = getattr(loader, "dataset", None)
        fused = hasattr(self._model, "train_strict") and next(self._model.parameters()).is_cuda
        in_memory = hasattr(ds, "_user_ids") and hasattr(ds, "seen_csr")
        shuffled = isinstance(getattr(loader, "sampler", None), RandomSampler)
        plain_loader = (type(getattr(loader, "batch_sampler", None)) is BatchSampler
                        and not getattr(loader, "drop_last", False))
        observed = bool(self._events.get("train")) or self._debug or bool(self._config.get("custom_engines"))
        mode = "api"
        if fused and in_memory and shuffled and plain_loader and not observed:
            mode = "strict"
            opt = self._optimizer
            group = opt.param_groups[0]
            if type(opt).__name__ == "SGD" and group.get("momentum", 0) == 0 and self._item_counts is None:
                from revisit_bpr.fast import lag_within_budget

                num_items = self._config["num_items"]
                period = max(1, int(num_items * math.log(num_items) / (loader.batch_size or 1))) * (loader.batch_size or 1)
                if lag_within_budget(float(group["lr"]), min(period, len(ds))):
                    mode = "stream"
        log.info("train_mode auto -> %s", mode)
        return mode

    def interrupt(self) -> None:
        for engine in self.trainer.engines.values():
            engine.interrupt()

    def clean(self) -> None:
        del self.trainer

    # ---- wiring -----------------------------------------------------------------------------
    def _build_trainer(self) -> Trainer:
        cfg = self._config
        trainer = Trainer(self._model, self._optimizer, self._accelerator,
                          custom_engines=cfg.get("custom_engines", {}))
        if self._train_mode == "api":
            if isinstance(self._adaptive_p, float):
                batch = self._datasets["train"].batch_size or 1
                every = max(1, int(cfg["num_items"] * math.log(cfg["num_items"]) / batch))
                trainer.add_event("train", Events.GET_BATCH_COMPLETED(every=every),
                                  lambda: self._sampler.update_stats())
            trainer.add_event("train", Events.GET_BATCH_COMPLETED, self._train_batch)
        trainer.add_event("eval", Events.GET_BATCH_COMPLETED, self._to_device)
        if self._skip_seen:
            trainer.add_event("eval", ModelEvents.FORWARD_COMPLETED, self._remove_seen_items)
        if self._debug:
            trainer.add_event("train", Events.ITERATION_COMPLETED(every=2000),
                              lambda engine: engine.terminate_epoch())
        trainer.add_event("eval", Events.EPOCH_STARTED, self._reset_eval_metrics)
        trainer.add_event("eval", Events.ITERATION_COMPLETED, self._update_eval_metrics)
        trainer.add_event("eval", Events.COMPLETED, self._log_eval)
        trainer.add_event("train", Events.EPOCH_STARTED, self._reset_train_metrics)
        trainer.add_event("train", Events.ITERATION_COMPLETED, self._update_train_metrics)
        trainer.add_event("train", Events.EPOCH_COMPLETED, self._log_train)
        for key, handlers in self._events.items():
            for event, handler in handlers:
                trainer.add_event(key, event, handler, accelerator=self._accelerator)
        self._best, self._bad_evals = None, 0
        return trainer

    # ---- whole epochs inside the library ------------------------------------------------------
    def _install_fast_epochs(self, max_iters: dict) -> dict:
        """train_mode "strict" / "stream": the train engine sees ONE pseudo-batch per epoch and its
        step runs the epoch through bpr_train_strict (same mini-batches as the per-batch loop) or
        StreamTrainer; events, eval engine, metrics and early stopping are unchanged."""
        from revisit_bpr import engine as eng

        model, dev = self._model, self._accelerator.device
        ds = self._datasets["train"].dataset
        if not hasattr(ds, "_user_ids") or not hasattr(model, "train_strict"):
            raise NotImplementedError("train_mode needs SparseSamplingInMemoryWithCollator data and "
                                      "the fused BPR model")
        batch = self._datasets["train"].batch_size or 1
        users = ds._user_ids.to(dev, torch.int32)
        items = ds._item_ids.to(dev, torch.int32)
        limit = max_iters.pop("train", None)
        adaptive = isinstance(self._adaptive_p, float)
        p = self._adaptive_p if adaptive else 0.01
        num_items = self._config["num_items"]
        every = max(1, int(num_items * math.log(num_items) / batch)) if adaptive else 0
        scalars = torch.zeros(4, device=dev)
        state = {"epoch": 0, "drawn": 0}
        gen = torch.Generator(device=dev).manual_seed(self._seed)
        stream = None
        plain_sgd = True
        if self._train_mode == "stream":
            from revisit_bpr.fast import BatchedStreamTrainer, StreamTrainer

            opt = self._optimizer
            group = opt.param_groups[0]
            plain_sgd = type(opt).__name__ == "SGD" and group.get("momentum", 0) == 0
            indptr, indices = ds.seen_csr()
            kind = "adaptive" if adaptive else "uniform"
            if plain_sgd:  # the fused SGD kernel (immediate updates)
                stream = StreamTrainer(model, users, items, indptr.to(dev), indices.to(dev),
                                       lr=group["lr"], sampler=kind, adaptive_p=p, batch_size=batch,
                                       seed=self._seed, refresh_lag="auto")  # lag 1 only inside the staleness budget
            else:  # Adam / momentum / RMSprop / Adagrad: the batched STREAM kernel (virtual mini-batches)
                stream = BatchedStreamTrainer(model, opt, users, items, indptr.to(dev),
                                              indices.to(dev), sampler=kind, adaptive_p=p,
                                              batch_size=batch, seed=self._seed)

        def epoch_step(engine, _batch) -> dict:
            model.train()
            if stream is not None:
                if plain_sgd:
                    stream.engine.set_optimizer(eng.OPT_SGD, lr=self._optimizer.param_groups[0]["lr"])
                m = stream.train_epoch()
                n_batches = max(1, math.ceil(m["triples"] / batch))
                out = {k: torch.tensor(m[k] * m["triples"] / n_batches, device=dev)
                       for k in ("bpr_loss", "l2_reg")}
                out["logits"] = torch.tensor([m["logits_diff"]], device=dev)
            else:
                perm = torch.randperm(users.numel(), device=dev, generator=gen)
                if limit is not None:
                    perm = perm[:limit * batch]
                if adaptive and state["epoch"] == 0:
                    # once, as the reference does before training (exp.py:129-132); afterwards the
                    # sampler's own counter, which keeps counting across epochs, drives the refresh
                    model.engine().adaptive_refresh()
                scalars.zero_()
                steps = model.train_strict(self._optimizer, users[perm].contiguous(),
                                           items[perm].contiguous(), batch,
                                           eng.NEG_ADAPTIVE if adaptive else eng.NEG_UNIFORM,
                                           adaptive_p=p, seed=self._seed, offset=state["drawn"],
                                           refresh_every=every, scalars=scalars)
                state["drawn"] += perm.numel()
                sc = scalars.tolist()
                out = {"bpr_loss": torch.tensor(sc[0] / steps, device=dev),
                       "l2_reg": torch.tensor(sc[1] / steps, device=dev),
                       "logits": torch.tensor([sc[2] / max(sc[3], 1.0)], device=dev)}
            out["loss"] = out["bpr_loss"] + out["l2_reg"]
            engine.state.metrics["_loss"] += out["loss"]
            state["epoch"] += 1
            return out

        self.trainer.engines["train"]._process = epoch_step
        return {**self._datasets, "train": [{"epoch": True}]}

    # ---- the evaluation as ONE pass (r6) --------------------------------------------------------
    def _can_fuse_eval(self, max_iters: dict) -> bool:
        """The eval engine's per-batch loop — DataLoader -> [B, I] target + padded seen matrix on the host ->
        model(batch) -> 14 metric objects, each ranking the [B, I] scores again (exp.py:369-374 of the reference) —
        is replaced by `revisit_bpr.evaluation.evaluate_topk` (one GEMM + one top-k per block of users for every
        NDCG / Recall / Precision at every k; ROC-AUC by counting) when nothing can tell the difference: whole
        epochs already run inside the library, seen items are masked (`skip_seen`), the eval set is `InMemory`
        behind `AllItemsCollator`, every metric is one of those (NDCG with the default gain), nobody listens to
        the eval engine's iterations and no eval iteration cap is set."""
        from experiments.bpr.dataset import AllItemsCollator, InMemory
        from revisit_bpr.metrics import NDCG, Precision, Recall
        from revisit_bpr.metrics.auc import RocAucMany, RocAucManySlow

        loader = self._datasets.get("eval")
        if loader is None or not self._skip_seen or max_iters.get("eval") is not None or self._events.get("eval"):
            return False
        if not isinstance(getattr(loader, "dataset", None), InMemory) or \
                not isinstance(getattr(loader, "collate_fn", None), AllItemsCollator):
            return False
        for m in self._metrics.values():
            if isinstance(m, NDCG) and getattr(m, "_gain", "exp") != "exp":
                return False
            if not isinstance(m, (NDCG, Recall, Precision, RocAucMany, RocAucManySlow)):
                return False
        mf = getattr(self._model, "logits_model", None)
        return bool(self._metrics) and mf is not None and hasattr(mf, "get_features") and \
            mf.get_features().get("user_bias") is None and next(self._model.parameters()).is_cuda

    def _install_fast_eval(self, loaders: dict) -> dict:
        from revisit_bpr.evaluation import evaluate_topk
        from revisit_bpr.metrics import NDCG, Precision, Recall

        dev = self._accelerator.device
        ds = self._datasets["eval"].dataset
        num_users = self._config["num_users"]
        users = np.asarray([smp["user"] for smp in ds._samples], np.int64)
        tcnt = np.asarray([len(smp["item"]) for smp in ds._samples], np.int64)
        titems = np.concatenate([np.asarray(smp["item"], np.int64) for smp in ds._samples]) if len(users) else \
            np.zeros(0, np.int64)
        if len(np.unique(users)) != len(users):
            raise ValueError("fused evaluation: an eval user appears twice")
        scnt = np.zeros(num_users, np.int64)
        seen_rows = [np.asarray(ds._seen[int(u)], np.int64) for u in users]
        scnt[users] = [len(r) for r in seen_rows]
        order = np.argsort(users, kind="stable")
        sflat = np.concatenate([seen_rows[k] for k in order]) if len(users) else np.zeros(0, np.int64)
        t = {"users": torch.from_numpy(users.astype(np.int32)).to(dev),
             "eval_indptr": torch.from_numpy(np.concatenate([[0], np.cumsum(tcnt)])).to(dev),
             "eval_items": torch.from_numpy(titems.astype(np.int32)).to(dev),
             "seen_indptr": torch.from_numpy(np.concatenate([[0], np.cumsum(scnt)])).to(dev),
             "seen_indices": torch.from_numpy(sflat.astype(np.int32)).to(dev)}
        names = {}
        for name, m in self._metrics.items():
            names[name] = (f"ndcg@{m._topk}" if isinstance(m, NDCG) else f"recall@{m._topk}" if isinstance(m, Recall)
                           else f"precision@{m._topk}" if isinstance(m, Precision) else "auc")
        ks = tuple(sorted({m._topk for m in self._metrics.values() if hasattr(m, "_topk")})) or (1,)
        want_auc = "auc" in names.values()

        def eval_step(engine, _batch) -> dict:
            self._model.eval()
            f = self._model.logits_model.get_features()
            out = evaluate_topk(f["user"].detach(), f["item"].detach(),
                                None if f.get("item_bias") is None else f["item_bias"].detach(), t["users"],
                                t["eval_indptr"], t["eval_items"], t["seen_indptr"], t["seen_indices"], ks=ks,
                                auc=want_auc)
            for name, key in names.items():
                engine.state.metrics[name] = torch.tensor(out[key], device=dev)
            return {}

        self.trainer.engines["eval"]._process = eval_step
        self._eval_fused = True
        log.info("evaluation fused into one pass over %d users (evaluate_topk)", len(users))
        return {**loaders, "eval": [{"epoch": True}]}

    # ---- handlers ---------------------------------------------------------------------------
    def _to_device(self, engine) -> None:
        dev = self._accelerator.device
        engine.state.batch = {k: (v.to(dev) if torch.is_tensor(v) else v)
                              for k, v in engine.state.batch.items()}

    @torch.no_grad()
    def _train_batch(self, engine) -> None:
        self._to_device(engine)
        batch = engine.state.batch
        if batch["item"].dim() < 2:
            batch["item"] = batch["item"].unsqueeze(-1)
        batch["neg"] = self._sampler.sample(batch)

    def _remove_seen_items(self, engine) -> None:
        batch, output = engine.state.batch, engine.state.output
        seen = batch.get("seen_items")
        if seen is not None:
            output["logits"].scatter_(dim=-1, index=seen, value=-1e13)
            output["logits"][:, 0] = -1e13

    def _reset_eval_metrics(self, engine) -> None:
        for m in self._metrics.values():
            m.reset()

    def _update_eval_metrics(self, engine) -> None:
        batch, output = engine.state.batch, engine.state.output
        if "target" not in batch:
            return
        for name, m in self._metrics.items():
            if "mask" in batch and hasattr(m, "compute") and m.__class__.__name__.startswith("RocAuc"):
                m(output["logits"], batch["target"], batch["mask"])
            else:
                m(output["logits"], batch["target"])
            engine.state.metrics[name] = m.get_metric()

    def _reset_train_metrics(self, engine) -> None:
        for key in ("bpr_loss", "l2_reg", "logits_diff"):
            engine.state.metrics[f"_{key}"] = torch.tensor(0.0, device=self._accelerator.device)

    @torch.no_grad()
    def _update_train_metrics(self, engine) -> None:
        st, out = engine.state, engine.state.output
        for key in ("bpr_loss", "l2_reg"):
            st.metrics[f"_{key}"] += out[key]
            st.metrics[key] = st.metrics[f"_{key}"] / st.epoch_iteration
        st.metrics["_logits_diff"] += out["logits"].abs().mean()
        st.metrics["logits_diff"] = st.metrics["_logits_diff"] / st.epoch_iteration

    @staticmethod
    def _public(metrics: dict) -> dict:
        return {k: (float(v) if torch.is_tensor(v) else v) for k, v in metrics.items()
                if not k.startswith("_")}

    def _log_train(self, engine) -> None:
        row = {"engine": "train", "epoch": engine.state.epoch, "t": time.perf_counter(), **self._public(engine.state.metrics)}
        self.history.append(row)
        log.info("train epoch %d | %s", engine.state.epoch,
                 " ".join(f"{k}={v:.4f}" for k, v in row.items() if isinstance(v, float)))

    def _log_eval(self, engine) -> None:
        train_epoch = self.trainer.engines["train"].state.epoch
        row = {"engine": "eval", "epoch": train_epoch, "t": time.perf_counter(), **self._public(engine.state.metrics)}
        self.history.append(row)
        log.info("eval before epoch %d | %s", train_epoch,
                 " ".join(f"{k}={v:.4f}" for k, v in row.items() if isinstance(v, float)))
        name, patience, direction = self._early
        if name is None or name not in row:
            return
        value = row[name] if direction == "max" else -row[name]
        if self._best is None or value > self._best:
            self._best, self._bad_evals = value, 0
        else:
            self._bad_evals += 1
            if self._bad_evals >= patience:
                log.info("early stopping on %s", name)
                self.trainer.engines["train"].terminate()
