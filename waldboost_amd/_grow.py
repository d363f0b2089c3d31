"""What the two tree learners share on the host (``training.DTree.fit``: CART on float32, csrc/wb_cart.hip;
``fpga.DTree.fit``: information gain on uint8 histograms, csrc/wb_fit.hip): the weight check, the staging
of the samples on the device and ``grow``, the level-by-level growth loop.  ``grow`` knows nothing of either learner, of
torch or of the native library; a learner hands it four callables:

    new_node(samples, depth, **extra) -> dict: a node over the ascending sample indices; the loop adds ``id`` (level
        order) and ``left`` = ``right`` = -1
    opens(node) -> bool: whether the node is searched for a split (the learner's leaf rules)
    search(depth, level, opened, child_base) -> (records, where): the split search of one level, the only step that touches
        the GPU.  `level` are the level's nodes, `opened` those among them that opened, in order; records[j] belongs to
        opened[j]; where[i] is the int32 node id of sample i after the level: child_base + 2 * j for a sample of opened[j]
        that went left, child_base + 2 * j + 1 for one that went right
    split(node, record) -> None | (extra, extra): what a record means.  None leaves the node a leaf; otherwise the node
        takes its split from the record and the pair is handed to new_node for the left and the right child
"""
import numpy as np

from ._native import is_tensor

MAX_DEPTH = 4           # a level holds at most WB_FIT_MAX_OPEN = 8 open nodes: depths 0 .. 3 are split


def check_weights(W, n, name):
    W = np.asarray(W)
    if W.ndim != 1 or W.size != n:
        raise ValueError(f"{name} must hold one weight per sample ({n}), got shape {W.shape}")
    if W.dtype.kind != "f":
        W = W.astype(np.float64)
    if not np.all(np.isfinite(W)) or np.any(W < 0):
        raise ValueError(f"{name} must be finite and non-negative")
    return W


def stage(X0, X1, F, dtype, q, Y, dev):
    """(xt, q_d, cls_d, node_d) on the device: the samples of both classes as one feature-major tensor (F, N) of `dtype`
    (a column is contiguous), the integer weights, the classes, and every sample's node id (0: the root)."""
    import torch
    parts = [(X if is_tensor(X) else torch.from_numpy(np.ascontiguousarray(X))).to(dev).reshape(int(X.shape[0]), F) for X in (X0, X1)]
    xt = torch.cat(parts).to(dtype).t().contiguous()
    return (xt, torch.from_numpy(q.view(np.int64)).to(dev), torch.from_numpy(Y.astype(np.uint8)).to(dev),
            torch.zeros(Y.size, dtype=torch.int32, device=dev))


def grow(n_samples, new_node, opens, search, split):
    """Grow a tree level by level until a level opens no node -> {level-order id: node}, in order of creation."""
    nodes = {0: dict(new_node(np.arange(n_samples), 0), id=0, left=-1, right=-1)}
    level, next_id, depth = [nodes[0]], 1, 0
    while True:
        opened = [nd for nd in level if opens(nd)]
        if not opened:
            return nodes
        records, where = search(depth, level, opened, next_id)
        level = []
        for j, nd in enumerate(opened):
            extras = split(nd, records[j])
            if extras is None:
                continue
            nd["left"], nd["right"] = next_id + 2 * j, next_id + 2 * j + 1
            for cid, extra in zip((nd["left"], nd["right"]), extras):
                nodes[cid] = dict(new_node(np.flatnonzero(where == cid), depth + 1, **extra), id=cid, left=-1, right=-1)
                level.append(nodes[cid])
        next_id += 2 * len(opened)
        depth += 1
