"""How the loaders hand host data to the device: one ring of pinned buffers, one packed upload, one prefetch loop.

The upload of a batch's tables is asynchronous, so a pinned staging buffer may only be rewritten once the copy that read it
has run (a single reused buffer let frame k be cropped with frame k + 1's boxes whenever the stream was running behind).
`PinnedRing` is that rule, once: NBUF buffers in rotation, each guarded by the event recorded after its last upload.
`FrameCropper` and `DetectionArena.fill` use the ring alone.

`upload` puts several host arrays into ONE pinned copy (`pack`: every part 16-byte aligned, which the decode's tables need
and every other consumer is satisfied by) and returns typed views of the device copy.

`StagedLoader` is what `GpuAugmentLoader`, `GpuDetectionLoader` and `ArenaDetectionLoader` share: the ring, the choice of
stream -- the consumer's current one, or with `prefetch` >= 1 a copy stream of the loader's own -- and the loop that keeps
`prefetch` + 1 batches enqueued and hands each over with an event the consumer's stream waits on.  The yielded tensors belong
to the consumer (fresh allocations, recorded on the consumer's stream); only the pinned staging rotates."""
import collections

import torch

__all__ = ['PinnedRing', 'pack', 'upload', 'device_parts', 'StagedLoader', 'ALIGN']

ALIGN = 16


class _Slot:
    host = event = None         # pinned uint8 tensor; event recorded behind the last copy that read it

    def uploaded(self, stream):
        """The copy that reads `host` has been enqueued on `stream`: the slot is not handed out again before it has run."""
        self.event = torch.cuda.Event()
        self.event.record(stream)


class PinnedRing:
    NBUF = 3

    def __init__(self, min_bytes):
        self.min_bytes = int(min_bytes)
        self._slots = [_Slot() for _ in range(self.NBUF)]
        self._turn = 0

    def take(self, nbytes):
        """-> the next slot, its `host` a pinned uint8 tensor of at least `nbytes`, once the upload that last read it has
        completed.  The caller fills it, enqueues its copy and calls `slot.uploaded(stream)`."""
        slot = self._slots[self._turn]
        self._turn = (self._turn + 1) % self.NBUF
        if slot.event is not None:
            slot.event.synchronize()
        if slot.host is None or slot.host.numel() < nbytes:
            slot.host = torch.empty(max(nbytes, self.min_bytes), dtype=torch.uint8).pin_memory()
        return slot


def pack(parts, align=ALIGN):
    """Pure numpy: uint8 arrays (or their sizes) -> (offset of each in one buffer, every offset a multiple of `align`; bytes of
    that buffer)."""
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total += -(-getattr(p, 'size', p) // align) * align
    return offs, total


class _Uploaded:
    """The device copy of packed parts: `meta`, the one uint8 allocation, and typed views of its parts."""

    def __init__(self, meta, offs, sizes):
        self.meta, self._offs, self._sizes = meta, offs, sizes

    def part(self, k, dtype, *shape):
        o = self._offs[k]
        return self.meta[o:o + self._sizes[k]].view(dtype).view(*shape)


def upload(ring, parts, stream, device):
    """parts: uint8 arrays -> their copy in a fresh device tensor, through the ring's next slot and one `non_blocking` copy
    enqueued on `stream`."""
    offs, total = pack(parts)
    slot = ring.take(total)
    host = slot.host.numpy()
    for p, o in zip(parts, offs):
        host[o:o + p.size] = p
    with torch.cuda.stream(stream):
        meta = torch.empty(max(total, ALIGN), dtype=torch.uint8, device=device)
        meta[:total].copy_(slot.host[:total], non_blocking=True)
    slot.uploaded(stream)
    return _Uploaded(meta, offs, [p.size for p in parts])


def device_parts(sizes, device):
    """-> uint8 views of these sizes, laid out by `pack`, in ONE fresh device tensor on the current stream: the outputs of a
    launch that writes several tables."""
    offs, total = pack(sizes)
    res = torch.empty(total, dtype=torch.uint8, device=device)
    return [res[o:o + n] for o, n in zip(offs, sizes)]


class StagedLoader:
    """The base of the loaders that finish their batches on the device (the module's docstring).  A subclass enqueues one
    batch on `self._stream(device, prefetch)`, uploads its tables with `upload(self._ring, ...)` and returns
    `(tensors, self._ready(stream, prefetch))`; its `__iter__` is `self._batches(source, enqueue)`."""

    def __init__(self, prefetch, min_staging):
        self.prefetch = int(prefetch)
        self._ring = PinnedRing(min_staging)
        self._copy_stream = None

    def _stream(self, device, prefetch):
        """The stream a batch is enqueued on: the copy stream (prefetch >= 1) or the caller's current stream (prefetch 0)."""
        if prefetch > 0:
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=device)
            return self._copy_stream
        return torch.cuda.current_stream(device)

    @staticmethod
    def _ready(stream, prefetch):
        """The event a consumer waits on before it reads a batch enqueued on the copy stream; None on its own stream."""
        if prefetch <= 0:
            return None
        ready = torch.cuda.Event()
        ready.record(stream)
        return ready

    @staticmethod
    def _public(tensors, ready):
        """What the public `finish` returns: the tensors, the ready event appended when there is one."""
        return tensors if ready is None else tensors + (ready,)

    def _batches(self, source, enqueue):
        """source: an iterator of what `enqueue` takes; enqueue(item, (batch number,)) -> (tensors, ready event or None).
        Keeps `self.prefetch` + 1 batches enqueued (the attribute is read at every step: it may be set between epochs) and
        yields each batch's tensors once the consumer's stream waits for it."""
        pending, done, b = collections.deque(), False, 0
        while True:
            while not done and len(pending) <= self.prefetch:
                try:
                    item = next(source)
                except StopIteration:
                    done = True
                    break
                pending.append(enqueue(item, (b,)))
                b += 1
            if not pending:
                return
            out, ready = pending.popleft()
            if ready is not None:
                consumer = torch.cuda.current_stream(out[0].device)
                consumer.wait_event(ready)
                for t in out[:2]:                # (everything behind the images shares one allocation)
                    t.record_stream(consumer)
            yield out
