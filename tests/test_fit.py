"""GPU checks of train.fit: the device-resident training loop (EpochLog's fused
epoch tail, the gated Adam, one captured epoch replayed) against the loop
written by hand -- tests/test_native_train_step.py's native_train_run shape:
train.Adam, train.IndexedCrossEntropy, metrics.evaluate_with_loss and
oracle.gcn_ref.EarlyStopping, one host decision per epoch.

The hand-written loop is documented as bitwise reproducible; every comparison
first asserts that two runs of it agree, then holds fit to it BITWISE: the stop
epoch, every history entry, every parameter, exp_avg, exp_avg_sq and the
optimiser's step count.  The small graph is where the loop logic is under test
(the kernels have their own files); R8 runs once.  Against the reference's own
runs (tests/golden r8_meta.json train_runs) fit is held to the bounds of
test_r8_native_training_matches_the_reference_run."""
import functools

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, datasets, metrics, train
from oracle import gcn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def small():
    """About 300 documents + 10 topics, 60 features, 4 classes a GCN can learn (the class of a document's
    strongest topic), 200 training and 100 validation documents."""
    g = datasets.doc_topic_graph(300, 10, 4, seed=3, emb_dim=60)
    assert g["nfeat"] == 60 and g["nodes"] == 310
    target = (np.argmax(g["features_dense"][:300, :10], axis=1) % 4).astype(np.int64)
    perm = np.random.default_rng(4).permutation(300)
    return {"features": g["features"].to(DEV), "adj": g["adj"].to(DEV), "target": torch.from_numpy(target).to(DEV),
            "train_idx": torch.from_numpy(perm[:200]).to(DEV), "val_idx": torch.from_numpy(perm[200:]).to(DEV),
            "nfeat": 60, "nclass": 4, "nodes": 310}


def make_model(d, seed, nhid, dropout, rng):
    torch.manual_seed(seed)                                 # trainer.py:295
    np.random.seed(seed)                                    # trainer.py:296
    return GCN(nfeat=d["nfeat"], nhid=nhid, nclass=d["nclass"], dropout=dropout, dropout_rng=rng).to(DEV)


def hand_loop(d, seed, nhid=16, dropout=0.5, rng="device", lr=0.02, max_epoch=200, patience=10):
    """trainer.py:349-376 on the native loss, optimiser and metrics, deciding on the host after every
    epoch: (history, model, optimiser)."""
    model = make_model(d, seed, nhid, dropout, rng)
    opt = train.Adam(model.parameters(), lr=lr)             # trainer.py:308
    crit = train.IndexedCrossEntropy()                      # trainer.py:307
    stopper = gcn_ref.EarlyStopping(patience)
    history = []
    for epoch in range(max_epoch):                          # trainer.py:349-376
        model.train()
        opt.zero_grad()
        loss = crit(model(d["features"], d["adj"]), d["target"], d["train_idx"])
        loss.backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            acc, f1, p, r, vl = metrics.evaluate_with_loss(model(d["features"], d["adj"]), d["target"], d["val_idx"],
                                                           d["nclass"])
        history.append({"epoch": epoch, "train_loss": loss.item(), "val_loss": vl, "acc": acc, "macro_f1": f1,
                        "precision": p, "recall": r})
        if stopper(vl):
            break
    return history, model, opt


def fit_run(d, seed, nhid=16, dropout=0.5, rng="device", lr=0.02, max_epoch=200, patience=10, **kw):
    model = make_model(d, seed, nhid, dropout, rng)
    res = train.fit(model, d["features"], d["adj"], d["target"], d["train_idx"], d["val_idx"], lr=lr,
                    max_epoch=max_epoch, patience=patience, **kw)
    return res, model


def bits(x):
    return np.float64(x).view(np.int64)


def same_history(a, b):
    return len(a) == len(b) and all(
        ha.keys() == hb.keys() and ha["epoch"] == hb["epoch"] and
        all(bits(ha[k]) == bits(hb[k]) for k in ha if k != "epoch") for ha, hb in zip(a, b))


def same_model(ma, oa, mb, ob):
    if oa.steps != ob.steps:
        return False
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        if not torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)):
            return False
        for k in ("exp_avg", "exp_avg_sq"):
            if not torch.equal(oa.state[pa][k].view(torch.int32), ob.state[pb][k].view(torch.int32)):
                return False
    return True


def hold_to_the_loop(d, label, fit_kw, **hyper):
    h1, m1, o1 = hand_loop(d, **hyper)
    h2, m2, o2 = hand_loop(d, **hyper)
    assert same_history(h1, h2) and same_model(m1, o1, m2, o2), f"{label}: the hand-written loop does not repeat"
    res, mf = fit_run(d, **hyper, **fit_kw)
    print(f"{label}: loop {len(h1)} epochs, last {h1[-1]}; fit {res.epochs} epochs, stop reason {res.stop_reason}, "
          f"optimiser steps {res.optimizer.steps} (loop {o1.steps})")
    assert res.epochs == len(h1) == len(res.history), f"{label}: fit stopped at another epoch"
    assert same_history(res.history, h1), f"{label}: a history entry differs"
    assert res.optimizer.steps == o1.steps == len(h1)
    assert same_model(mf, res.optimizer, m1, o1), f"{label}: a parameter or moment differs"
    st = res.log.state()
    assert (st.epoch, st.stop_epoch, st.stopped, st.arrivals) == (len(h1), len(h1) - 1, res.stop_reason, 0)
    assert not mf.training
    return h1, res


# seed, patience: the loop stops early, and not on the last epoch of a group of 7 replays (epoch 0 is
# eager, so a poll follows the epochs 7, 14, ...): epochs queued behind the stop run gated
SMALL = dict(seed=11, nhid=16, dropout=0.5, rng="device", lr=0.02, max_epoch=200, patience=3)


def test_graph_fit_is_bitwise_the_hand_written_loop_small_graph():
    h, res = hold_to_the_loop(small(), "small graph", dict(graph=True, poll_every=7), **SMALL)
    assert len(h) < SMALL["max_epoch"] and res.stop_reason == 1, "the loop must stop early"
    assert (len(h) - 1) % 7 != 0, "the stop must fall inside a group of replays, so that the gate is exercised"
    assert len(h) > 8, "at least one whole group of replays before the stop"


def test_graph_fit_reaching_max_epoch_before_patience():
    hyper = dict(SMALL, max_epoch=5, patience=50)
    h, res = hold_to_the_loop(small(), "max_epoch first", dict(graph=True, poll_every=7), **hyper)
    assert len(h) == 5 and res.stop_reason == 2


def test_eager_fit_polling_every_epoch_is_bitwise_the_hand_written_loop():
    d = small()
    h, res = hold_to_the_loop(d, "eager", dict(graph=False, poll_every=1), **SMALL)
    assert res.stop_reason == 1
    # with one look per epoch nothing runs behind the stop: the mask offset is the loop's too
    _, m, _ = hand_loop(d, **SMALL)
    _, mf = fit_run(d, **SMALL, graph=False, poll_every=1)
    assert int(mf._rng_base.item()) == int(m._rng_base.item()) == len(h) * d["nodes"] * SMALL["nhid"]


def test_graph_fit_is_bitwise_the_hand_written_loop_r8(r8, golden_meta):
    run = golden_meta["train_runs"]["50494"]
    d = {"features": r8["features"].to(DEV), "adj": r8["adj"].to(DEV),
         "target": torch.as_tensor(r8["target"]).long().to(DEV),
         "train_idx": torch.as_tensor(run["train_idx"]).long().to(DEV),
         "val_idx": torch.as_tensor(run["val_idx"]).long().to(DEV),
         "nfeat": r8["nfeat"], "nclass": r8["nclass"], "nodes": r8["nodes"]}
    h, res = hold_to_the_loop(d, "R8", dict(graph=True, poll_every=7), seed=50494, nhid=200, dropout=0.5,
                              rng="device", lr=0.02, max_epoch=200, patience=3)
    assert len(h) < 200 and res.stop_reason == 1


@pytest.mark.parametrize("seed", [50494, 99346])
def test_r8_fit_matches_the_reference_run(r8, golden_meta, seed):
    """fit with the default CPU masks (eager, one look per epoch) against the reference's own run, to
    test_r8_native_training_matches_the_reference_run's bounds."""
    run = golden_meta["train_runs"][str(seed)]
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = GCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5).to(DEV)
    features, adj = r8["features"].to(DEV), r8["adj"].to(DEV)
    target = torch.as_tensor(r8["target"]).long().to(DEV)
    res = train.fit(model, features, adj, target, run["train_idx"], run["val_idx"], lr=0.02, max_epoch=200,
                    patience=10)
    assert not model.training
    with torch.no_grad():
        acc = metrics.evaluate_with_loss(model(features, adj), target,
                                         torch.as_tensor(r8["test_lst"]).long().to(DEV), r8["nclass"])[0]
    for h, g in list(zip(res.history, run["history"]))[:10]:
        print(f"seed {seed} epoch {h['epoch']}: train loss {h['train_loss']:.6f} reference {g['train_loss']:.6f} "
              f"val loss {h['val_loss']:.6f} reference {g['val_loss']:.6f}")
    print(f"seed {seed}: test acc {acc:.6f} reference {run['test']['acc']:.6f} epochs {res.epochs} "
          f"reference {len(run['history'])}")
    assert abs(acc - run["test"]["acc"]) <= 0.001 + 1e-12, (acc, run["test"]["acc"], res.epochs)
    assert len(res.history) >= 10
    for h, g in list(zip(res.history, run["history"]))[:10]:
        assert abs(h["train_loss"] - g["train_loss"]) < 1e-3


def test_a_captured_epoch_advances_the_state_and_the_masks_on_every_replay():
    d = small()
    N, nhid = 5, 16
    model = make_model(d, 7, nhid, 0.5, "device")
    log = train.EpochLog(100, d["nclass"], DEV, patience=1000)
    opt = train.Adam(model.parameters(), lr=0.02, gate=log.stop_word)
    args = (model, d["features"], d["adj"], d["target"], d["train_idx"], d["val_idx"], opt, log)
    train.run_epoch(*args)   # eager: plans, records, row counts
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        train.run_epoch(*args)
    e0, base0, steps0 = log.poll()[0], int(model._rng_base.item()), opt.steps
    assert (e0, steps0) == (1, 1)   # the capture ran nothing
    for _ in range(N):
        g.replay()
    torch.cuda.synchronize()
    assert log.poll() == (1 + N, 0)
    assert int(model._rng_base.item()) - base0 == N * d["nodes"] * nhid
    assert opt.steps == 1 + N
    hist = log.history()
    assert [h["epoch"] for h in hist] == list(range(1 + N))
    assert len({h["train_loss"] for h in hist}) == 1 + N   # every replay trained on: a new loss each epoch
    del g


def test_contracts():
    d = small()
    model = make_model(d, 1, 16, 0.5, "cpu")
    with pytest.raises(ValueError, match="graph=True"):
        train.fit(model, d["features"], d["adj"], d["target"], d["train_idx"], d["val_idx"], graph=True)
    model = make_model(d, 1, 16, 0.5, "device")
    # the labels cover the 300 documents: a topic node (row 305) has none
    for tr, va in ((torch.tensor([1, 2, 305]), d["val_idx"]), (d["train_idx"], torch.tensor([3, 305]))):
        with pytest.raises(IndexError, match="outside"):
            train.fit(model, d["features"], d["adj"], d["target"], tr, va, max_epoch=3)
    with pytest.raises(ValueError, match="poll_every"):
        train.fit(model, d["features"], d["adj"], d["target"], d["train_idx"], d["val_idx"], poll_every=0)
    # dropout 0 needs no masks at all: the graph path is open to the default dropout_rng
    torch.manual_seed(1)
    model = GCN(nfeat=d["nfeat"], nhid=16, nclass=d["nclass"], dropout=0.0).to(DEV)
    res = train.fit(model, d["features"], d["adj"], d["target"], d["train_idx"], d["val_idx"], max_epoch=4,
                    patience=50, graph=True, poll_every=2)
    assert (res.epochs, res.stop_reason, res.optimizer.steps) == (4, 2, 4)
