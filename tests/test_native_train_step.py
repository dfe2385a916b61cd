"""The reference's training loop (trainer.py:349-406) with every call site on
native code: the drop-in GCN with the reference's dropout stream,
train.IndexedCrossEntropy for nn.CrossEntropyLoss (trainer.py:307, 358),
train.Adam for th.optim.Adam (trainer.py:308, 362) and
metrics.evaluate_with_loss for the validation loss and metrics
(trainer.py:378-398), on R8 for the two golden seeds -- held to the bounds of
test_r8_training_accuracy_parity: test accuracy within +-0.1 % of the
reference's run, train loss within 1e-3 of its history for the first 10 epochs."""
import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, metrics, train
from oracle import gcn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def native_train_run(features, adj, target, train_idx, val_idx, test_idx, nfeat, nclass, seed,
                     nhid=200, dropout=0.5, lr=0.02, max_epoch=200, patience=10):
    """trainer.py:294-406 for one seed (oracle/gcn_ref.py train_run's loop) on the native loss,
    optimiser and metrics: (history, test_desc)."""
    torch.manual_seed(seed)                                 # trainer.py:295
    np.random.seed(seed)                                    # trainer.py:296
    model = GCN(nfeat=nfeat, nhid=nhid, nclass=nclass, dropout=dropout).to(DEV)
    opt = train.Adam(model.parameters(), lr=lr)             # trainer.py:308
    crit = train.IndexedCrossEntropy()                      # trainer.py:307
    features, adj = features.to(DEV), adj.to(DEV)
    target = torch.as_tensor(target).long().to(DEV)
    tr, va, te = (torch.as_tensor(i).long().to(DEV) for i in (train_idx, val_idx, test_idx))
    stopper = gcn_ref.EarlyStopping(patience)
    history = []

    def evaluate(idx, prefix):                              # trainer.py:378-398
        model.eval()
        with torch.no_grad():
            logits = model(features, adj)
            acc, f1, p, r, loss = metrics.evaluate_with_loss(logits, target, idx, nclass)
        return {f"{prefix}_loss": loss, "acc": acc, "macro_f1": f1, "precision": p, "recall": r}

    for epoch in range(max_epoch):                          # trainer.py:349-376
        model.train()
        opt.zero_grad()
        logits = model(features, adj)
        loss = crit(logits, target, tr)                     # trainer.py:358
        loss.backward()
        opt.step()
        desc = dict(epoch=epoch, train_loss=loss.item(), **evaluate(va, "val"))
        history.append(desc)
        if stopper(desc["val_loss"]):
            break
    return history, evaluate(te, "test")


@pytest.mark.parametrize("seed", [50494, 99346])
def test_r8_native_training_matches_the_reference_run(r8, golden_meta, seed):
    run = golden_meta["train_runs"][str(seed)]
    hist, test = native_train_run(r8["features"], r8["adj"], r8["target"], run["train_idx"], run["val_idx"],
                                  r8["test_lst"], r8["nfeat"], r8["nclass"], seed)
    for h, g in list(zip(hist, run["history"]))[:10]:
        print(f"seed {seed} epoch {h['epoch']}: train loss {h['train_loss']:.6f} reference {g['train_loss']:.6f} "
              f"val loss {h['val_loss']:.6f} reference {g['val_loss']:.6f}")
    print(f"seed {seed}: test acc {test['acc']:.6f} reference {run['test']['acc']:.6f} epochs {len(hist)} "
          f"reference {len(run['history'])}")
    assert abs(test["acc"] - run["test"]["acc"]) <= 0.001 + 1e-12, (test["acc"], run["test"]["acc"], len(hist))
    for h, g in list(zip(hist, run["history"]))[:10]:
        assert abs(h["train_loss"] - g["train_loss"]) < 1e-3
