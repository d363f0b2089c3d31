"""The schedule of Model.detect_stream: which image goes to which lane, when a batch is sent and when a lane is
collected.  No GPU code: a lane is anything with

    n_levels                               levels of its pyramid (0: nothing to scan)
    scan_image(image, dm, nms) -> token    one image loaded and its whole step enqueued        (batch == 1)
    load_slot(b, image)                    one image into slot b of the lane's batch           (batch > 1)
    scan_batch(dm, nms) -> token           the step over the loaded slots enqueued             (batch > 1)
    collect(owner, dm, token, count, nms)  the wait -> [result of image b for b < count]
    wait_upload()                          the last loaded image has left the caller's buffer
    synchronize()                          everything enqueued on the lane has run

(dm: the cascade to scan; nms: the call's suppression arguments; owner: the model the results are counted on).
Model.detect_stream's lanes wrap (PyramidEngine, torch.cuda.Stream); the host tests' lanes log their calls."""
import dataclasses
from typing import NamedTuple


@dataclasses.dataclass(eq=False)
class Filling:
    """The batch being gathered on a lane."""
    key: tuple                       # what its images share: shape, dtype, channel options
    lane: object
    dm: object
    count: int = 0                   # images loaded so far


class Sent(NamedTuple):
    """A lane whose step is enqueued and not yet collected."""
    lane: object
    dm: object
    token: object                    # what the lane's scan_* returned, for its collect
    count: int                       # images in it


class Schedule:
    """One detect_stream call over `lanes` lanes of `batch` images.
    pool: key -> [lane], kept between calls by the caller and bounded to two keys here; new_lane(key, image) builds a
    lane; direct(image) is the result of an image no lane can scan (no pyramid level)."""

    def __init__(self, pool, lanes, batch, new_lane, direct, owner, nms):
        self.pool, self.lanes, self.batch, self.new_lane, self.direct = pool, lanes, batch, new_lane, direct
        self.owner, self.nms = owner, nms
        self.pending = []            # [Sent], oldest first

    def _free_lane(self, key, image):
        """A lane of `key`'s group that no pending item holds (fewer than `lanes` are pending here)."""
        group = self.pool.get(key)
        if group is None:
            if len(self.pool) >= 2:
                self.pool.pop(next(iter(self.pool)))
            group = self.pool[key] = []
        for lane in group:
            for s in self.pending:
                if s.lane is lane:
                    break
            else:
                return lane
        group.append(self.new_lane(key, image))
        return group[-1]

    def _send(self, f):
        self.pending.append(Sent(f.lane, f.dm, f.lane.scan_batch(f.dm, self.nms), f.count))

    def _finish(self):
        s = self.pending.pop(0)
        return s.lane.collect(self.owner, s.dm, s.token, s.count, self.nms)

    def run(self, items):
        """items: (key, dm, image) per image, in order -> the images' results, in order."""
        pending, lanes, batch, nms = self.pending, self.lanes, self.batch, self.nms
        fill = None                                           # Filling: the lane being loaded
        try:
            for key, dm, image in items:
                if fill is not None and (fill.key != key or fill.dm is not dm):
                    self._send(fill)                          # (another shape, or the model changed: the batch goes as it is)
                    fill = None
                while len(pending) >= lanes:
                    yield from self._finish()
                if fill is None:
                    lane = self._free_lane(key, image)
                    if lane.n_levels == 0:
                        while pending:
                            yield from self._finish()
                        yield self.direct(image)
                        continue
                    fill = Filling(key, lane, dm)
                lane = fill.lane
                if batch == 1:
                    pending.append(Sent(lane, dm, lane.scan_image(image, dm, nms), 1))
                    fill = None
                else:
                    lane.load_slot(fill.count, image)
                    fill.count += 1
                    if fill.count == batch:
                        self._send(fill)
                        fill = None
                if len(pending) >= lanes:
                    yield from self._finish()
                # an image uploaded asynchronously from the caller's page-locked buffer: the copy has left that buffer
                # before the iterable is asked for its next image (a decoder may write into the same buffer again); by
                # now the scan is enqueued and an older lane has been collected, so this wait is over before it starts
                lane.wait_upload()
            if fill is not None:
                self._send(fill)
                fill = None
            while pending:
                yield from self._finish()
        finally:
            for s in pending:                                 # (the consumer stopped early: let the lanes drain)
                s.lane.synchronize()
            if fill is not None:
                fill.lane.synchronize()
