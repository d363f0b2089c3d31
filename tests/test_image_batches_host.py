"""samples.image_batches / stack_images (CPU): the one loop that groups an iterable of items into batches of one image
(shape, dtype) for DeviceSamplePool.update and calibration.prune_instances -- what it yields, and how far it has advanced
the caller's iterator when the caller stops after a group (DeviceSamplePool.update stops once its quotas are filled)."""
import numpy as np
import torch

from waldboost_amd.samples import image_batches, stack_images


def item(k, shape=(2, 3), dtype=np.uint8):
    return {"image": np.zeros(shape, dtype), "k": k}


def ids(groups):
    return [[it["k"] for it in g] for g in groups]


def test_groups():
    a = [item(k) for k in range(5)]
    assert ids(image_batches(a, 2)) == [[0, 1], [2, 3], [4]]                 # full batches, then the remainder
    assert ids(image_batches(a, 5)) == [[0, 1, 2, 3, 4]]                     # a full batch at the very end: no empty group after it
    assert ids(image_batches(a, 1)) == [[0], [1], [2], [3], [4]]
    assert ids(image_batches([], 3)) == [] and ids(image_batches(iter([]), 1)) == []
    # a shape change before the batch is full, and a dtype change at equal shape: what waits goes first
    b = [item(0), item(1), item(2, shape=(3, 2)), item(3, shape=(3, 2)), item(4, shape=(3, 2), dtype=np.float32), item(5)]
    assert ids(image_batches(b, 3)) == [[0, 1], [2, 3], [4], [5]]
    assert ids(image_batches(b, 2)) == [[0, 1], [2, 3], [4], [5]]             # the change right behind a full batch
    # a torch tensor is another kind than an ndarray of its shape ("torch.uint8" is not "uint8"), and stacks as a tensor
    c = [item(0), {"image": torch.zeros((2, 3), dtype=torch.uint8), "k": 1}, {"image": torch.ones((2, 3), dtype=torch.uint8), "k": 2}]
    groups = list(image_batches(c, 4))
    assert ids(groups) == [[0], [1, 2]]
    assert isinstance(stack_images(groups[0]), np.ndarray) and stack_images(groups[0]).shape == (1, 2, 3)
    stacked = stack_images(groups[1])
    assert isinstance(stacked, torch.Tensor) and tuple(stacked.shape) == (2, 2, 3) and stacked[1].sum() == 6
    assert stack_images(list(image_batches(a, 5))[0]).shape == (5, 2, 3)
    for g in image_batches(b, 3):                                            # one kind per group
        assert len({(it["image"].shape, str(it["image"].dtype)) for it in g}) == 1


def test_a_caller_that_stops_has_taken_what_the_loop_it_replaces_took():
    """The loop this generator replaces stood in DeviceSamplePool.update:

        for item in iterable:
            if group and kind(item) != kind_of_group:  flush(); break if the quotas are filled
            group.append(item)
            if len(group) == batch:                    flush(); break if the quotas are filled

    Full batch, batch 2, items 0 1 2 3 of one kind: items 0 and 1 are read, the group is full right behind the append of
    item 1 and is flushed before item 2 is read.  A caller that stops there finds item 2 next.
    Shape change, batch 3, items 0 1 of one kind and 2 3 of another: items 0, 1 and 2 are read; item 2 is of another kind,
    so [0, 1] is flushed, and a caller that stops there has lost item 2: it finds item 3 next."""
    it = iter([item(k) for k in range(4)])
    assert ids([next(image_batches(it, 2))]) == [[0, 1]]
    assert next(it)["k"] == 2
    it = iter([item(0), item(1), item(2, shape=(3, 2)), item(3, shape=(3, 2))])
    assert ids([next(image_batches(it, 3))]) == [[0, 1]]
    assert next(it)["k"] == 3
    # and one that goes on sees every item once
    it = iter([item(0), item(1), item(2, shape=(3, 2)), item(3, shape=(3, 2))])
    assert ids(image_batches(it, 3)) == [[0, 1], [2, 3]] and next(it, None) is None
