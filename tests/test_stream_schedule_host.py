"""CPU tests of waldboost_amd/stream.py: the schedule of Model.detect_stream on lanes that only log their calls.  What
detect_stream's docstring promises -- results in input order, at most lanes * batch - 1 images taken ahead, a shape or
model change sending a partly filled batch, a lane never loaded while pending, the lanes drained on an early close --
checked event by event."""
import itertools

import pytest

from waldboost_amd.stream import Schedule


class Boom(Exception):
    pass


class StubLane:
    """Logs ("load" | "scan" | "collect" | "wait_upload" | "synchronize", lane name, ...) into the shared log."""

    def __init__(self, log, name, n_levels, fail_on):
        self.log, self.name, self.n_levels, self.fail_on = log, name, n_levels, fail_on
        self.slots = {}

    def _load(self, b, image):
        self.log.append(("load", self.name, image))
        if image == self.fail_on:
            raise Boom(image)
        self.slots[b] = image

    def scan_image(self, image, dm, nms):
        self._load(0, image)
        return self.scan_batch(dm, nms)

    def load_slot(self, b, image):
        self._load(b, image)

    def scan_batch(self, dm, nms):
        assert nms == "nms"
        self.log.append(("scan", self.name, dm))
        return dict(self.slots)                               # (the token: what the slots held when the step was enqueued)

    def collect(self, owner, dm, token, count, nms):
        assert owner == "owner" and nms == "nms"
        self.log.append(("collect", self.name, count))
        return [("result", token[b], dm) for b in range(count)]

    def wait_upload(self):
        self.log.append(("wait_upload", self.name))

    def synchronize(self):
        self.log.append(("synchronize", self.name))


# the scripted sequence: 7 images of shapes A A A B B A A and one without a pyramid level (shape Z) among them
SHAPES = "AAABBZAA"


def sequence(model_change):
    """[(key, dm, image)]; model_change: the cascade is another object from the last image on."""
    return [(("shape", s), "dm1" if model_change and i == len(SHAPES) - 1 else "dm0", i) for i, s in enumerate(SHAPES)]


def play(lanes, batch, seq, stop_after=None, fail_on=None):
    """The schedule over `seq` -> (log, results, pool, the error that ended it); the log also holds ("pull", image) when
    the source is asked for an image and ("yield", image) when the consumer receives one's result."""
    log, pool, names = [], {}, itertools.count()

    def new_lane(key, image):
        return StubLane(log, f"{key[1]}{next(names)}", 0 if key[1] == "Z" else 3, fail_on)

    def source():
        for item in seq:
            log.append(("pull", item[2]))
            yield item

    gen = Schedule(pool, lanes, batch, new_lane, lambda image: ("direct", image), "owner", "nms").run(source())
    results, error = [], None
    try:
        for res in gen:
            log.append(("yield", res[1]))
            results.append(res)
            if len(results) == stop_after:
                break
    except Boom as e:
        error = e
    gen.close()
    return log, results, pool, error


def expected_batches(seq, batch):
    """Independent of the schedule: runs of one (key, dm), cut every `batch` images -> [[image]]; the image without levels
    ends a run and is in none."""
    out = []
    for (key, dm), run in itertools.groupby(seq, key=lambda it: it[:2]):
        run = [it[2] for it in run]
        if key[1] != "Z":
            out += [run[i:i + batch] for i in range(0, len(run), batch)]
    return out


def lane_states(log):
    """Replays the log: asserts that no lane is loaded while pending; -> (lanes pending at the end, lanes with images
    loaded and not scanned, synchronize calls per lane)."""
    pending, open_, syncs = set(), set(), {}
    for ev in log:
        kind, lane = ev[0], ev[1]
        if kind == "load":
            assert lane not in pending, f"{lane} loaded while pending"
            open_.add(lane)
        elif kind == "scan":
            assert lane not in pending
            open_.discard(lane)
            pending.add(lane)
        elif kind == "collect":
            assert lane in pending
            pending.discard(lane)
        elif kind == "synchronize":
            syncs[lane] = syncs.get(lane, 0) + 1
    return pending, open_, syncs


@pytest.mark.parametrize("model_change", [False, True])
@pytest.mark.parametrize("lanes,batch", [(3, 1), (2, 3), (1, 2)])
def test_whole_sequence(lanes, batch, model_change):
    seq = sequence(model_change)
    log, results, pool, error = play(lanes, batch, seq)
    assert error is None
    # results in input order, each from the cascade that was current when its image was taken
    assert results == [("direct", i) if key[1] == "Z" else ("result", i, dm) for key, dm, i in seq]
    # never more than lanes * batch - 1 images pulled ahead of the one yielded
    pulled = 0
    for ev in log:
        if ev[0] == "pull":
            pulled += 1
        elif ev[0] == "yield":
            assert pulled - (ev[1] + 1) <= lanes * batch - 1, f"{pulled} pulled when image {ev[1]} was yielded"
    # a partly filled batch goes at a shape or model change and at the end, with its true count
    want = expected_batches(seq, batch)
    assert any(len(b) < batch for b in want) or batch == 1
    assert [ev[2] for ev in log if ev[0] == "collect"] == [len(b) for b in want]
    loads = [ev[2] for ev in log if ev[0] == "load"]
    assert loads == [i for b in want for i in b]
    scans_after = [sum(1 for ev in log[:k] if ev[0] == "load") for k, ev in enumerate(log) if ev[0] == "scan"]
    assert scans_after == list(itertools.accumulate(len(b) for b in want))     # (each step enqueued right behind its last image)
    # no lane loaded while pending; everything collected, nothing left to drain
    pending, open_, syncs = lane_states(log)
    assert not pending and not open_ and not syncs
    # the upload wait follows the enqueue and precedes the next pull
    full = {b[-1] for b in want if len(b) == batch}
    pulls = [k for k, ev in enumerate(log) if ev[0] == "pull"]
    for k, k_next in zip(pulls, pulls[1:] + [len(log)]):
        image, seg = log[k][1], log[k:k_next]
        if seq[image][0][1] == "Z":
            assert not any(ev[0] in ("load", "wait_upload") for ev in seg)
            continue
        (at,) = [j for j, ev in enumerate(seg) if ev[:1] == ("load",) and ev[2] == image]
        lane = seg[at][1]
        (wait,) = [j for j, ev in enumerate(seg) if ev == ("wait_upload", lane)]
        assert wait > at
        if k_next < len(log):
            assert wait == len(seg) - 1                       # (the next image is asked for right after it)
        if image in full:
            (scan,) = [j for j, ev in enumerate(seg) if ev[:2] == ("scan", lane)]
            assert at < scan < wait
    assert len(pool) <= 2


@pytest.mark.parametrize("lanes,batch", [(3, 1), (2, 3), (1, 2)])
def test_a_consumer_that_stops_after_two_results(lanes, batch):
    log, results, pool, error = play(lanes, batch, sequence(False), stop_after=2)
    assert error is None and results == [("result", 0, "dm0"), ("result", 1, "dm0")]
    assert sum(1 for ev in log if ev[0] == "pull") <= 2 + lanes * batch - 1
    pending, open_, syncs = lane_states(log)
    # every pending lane and the open batch synchronised exactly once, no other lane
    # (one lane of two images: both results come from the one batch sent so far, nothing else is in flight)
    assert bool(pending | open_) == ((lanes, batch) != (1, 2)) and not pending & open_
    assert syncs == {lane: 1 for lane in pending | open_}
    assert [ev[0] for ev in log[len(log) - len(syncs):]] == ["synchronize"] * len(syncs)


@pytest.mark.parametrize("fail_on", [1, 4, 7])
@pytest.mark.parametrize("lanes,batch", [(3, 1), (2, 3), (1, 2)])
def test_a_lane_whose_load_raises(lanes, batch, fail_on):
    seq = sequence(False)
    log, results, pool, error = play(lanes, batch, seq, fail_on=fail_on)
    assert isinstance(error, Boom) and error.args == (fail_on,)
    # what was yielded before is a prefix of the right results; nothing is pulled after the failing image
    assert results == [("direct", i) if key[1] == "Z" else ("result", i, dm) for key, dm, i in seq][:len(results)]
    assert [ev[1] for ev in log if ev[0] == "pull"] == list(range(fail_on + 1))
    pending, open_, syncs = lane_states(log)
    assert open_ and syncs == {lane: 1 for lane in pending | open_}      # (the lane whose load failed among them)
    assert log[-1][0] == "synchronize"
