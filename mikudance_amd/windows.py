"""Frame windows for clips longer than the temporal context (host-side integer work).

Behavioural mirror of the reference's sliding-window scheduler (src/pipelines/context.py:7-49, called from
src/pipelines/pipeline_mikudance.py:577-589 as `scheduler(0, steps, F, context_frames, context_stride, context_overlap)`):
a clip that fits the context is one window; otherwise windows of `size` frames are laid out at dilations 1, 2, 4, ...
(`levels` of them), each level starting at a step-dependent phase and advancing by `size * dilation - overlap`, with
frame indices wrapping around the clip (closed loop).  The pipeline always passes step = 0, so the phase is 0 and the
same windows are used at every denoising step.  Pinned by tests/golden/g1_windows.json.

Two additions beside it (neither is the reference's; both opt-in):
  * WindowLayout.open_windows -- `context_schedule="uniform_open"`: the same levels and the same advance, but no window wraps round the
    end of the clip; the last window of a level is pulled back so that it ends on the last frame;
  * fuse_weights -- `context_fuse="pyramid"`: triangular per-slot weights, normalised per frame over all windows of the step."""
import math
from typing import Iterator, List


def bit_reversed_fraction(value: int, bits: int = 64) -> float:
    """value's `bits`-bit pattern mirrored and read as a binary fraction in [0, 1) (0 -> 0.0, 1 -> 0.5, 2 -> 0.25, ...)."""
    mirrored = 0
    for k in range(bits):
        if (value >> k) & 1:
            mirrored |= 1 << (bits - 1 - k)
    return mirrored / float(1 << bits)


class WindowLayout:
    """All windows of one denoising step."""

    def __init__(self, frames: int, size: int, max_levels: int, overlap: int, wrap: bool = True):
        self.frames, self.size, self.overlap, self.wrap = frames, size, overlap, wrap
        if frames > size and size - overlap <= 0:
            # the reference's range() would be given a step <= 0 here (src/pipelines/context.py:33-37): ValueError for 0,
            # an empty schedule (then a 0/0 average) for a negative one -- refuse both up front
            raise ValueError(f"context_overlap ({overlap}) must be smaller than context_frames ({size})")
        self.levels = 0 if frames <= size else min(max_levels, int(math.ceil(math.log2(frames / size))) + 1)

    def at_step(self, step: int) -> List[List[int]]:
        if self.frames <= self.size:
            return [list(range(self.frames))]
        phase = bit_reversed_fraction(step)
        shift = int(round(self.frames * phase))
        last = self.frames + shift - (0 if self.wrap else self.overlap)
        out = []
        for level in range(self.levels):
            dilation = 2 ** level
            first = int(phase * dilation) + shift
            advance = self.size * dilation - self.overlap
            span = self.size * dilation
            begin = first
            while begin < last:
                out.append([idx % self.frames for idx in range(begin, begin + span, dilation)])
                begin += advance
        return out

    def open_windows(self) -> List[List[int]]:
        """The open-ended layout: at dilation d = 2^level a window spans (size - 1) d + 1 frames and is range(begin, begin + span, d), no
        modulo.  Begins advance by size d - overlap from 0; the first one whose window would pass the end of the clip becomes frames - span
        and closes the level.  A level that does not fit into the clip ends the list; a window already emitted is not repeated."""
        if self.frames <= self.size:
            return [list(range(self.frames))]
        out = []
        for level in range(self.levels):
            dilation = 2 ** level
            span = (self.size - 1) * dilation + 1
            if span > self.frames:
                break
            advance = self.size * dilation - self.overlap
            begin = 0
            while True:
                last = begin + span >= self.frames
                if last:
                    begin = self.frames - span
                window = list(range(begin, begin + span, dilation))
                if window not in out:
                    out.append(window)
                if last:
                    break
                begin += advance
        return out


def iter_windows(step, frames, size, max_levels, overlap, wrap=True) -> Iterator[List[int]]:
    return iter(WindowLayout(frames, size, max_levels, overlap, wrap).at_step(step))


def iter_open_windows(frames, size, max_levels, overlap) -> Iterator[List[int]]:
    return iter(WindowLayout(frames, size, max_levels, overlap, wrap=False).open_windows())


def accumulate_slots(window: List[int]) -> List[int]:
    """The frame every slot of a window accumulates into: the frame itself, or -1 for an earlier occurrence of a frame that a wrapped,
    dilated window names twice (the reference's index_put keeps the LAST occurrence, src/pipelines/pipeline_mikudance.py:662-666)."""
    return [fr if fr not in window[j + 1:] else -1 for j, fr in enumerate(window)]


def pyramid(length: int) -> List[int]:
    """Triangular slot weights 1, 2, ..., peak, ..., 2, 1 of a window of `length` frames (the middle value once for odd, twice for even
    lengths): diffusers' FreeNoise weighting_scheme="pyramid"."""
    return [min(j + 1, length - j) for j in range(length)]


def fuse_weights(windows: List[List[int]], frames: int, fuse: str = "pyramid") -> List[List[float]]:
    """Per window, per slot: the slot's weight divided by the total weight its frame receives from every (window, slot) pair of the
    step, in float64 -- so a frame's shares sum to 1 and the accumulated buffer is the weighted mean.  Slots that do not accumulate
    (accumulate_slots: -1) weigh nothing and get 0."""
    if fuse != "pyramid":
        raise ValueError(f"fuse_weights: unknown weighting {fuse!r}")
    total = [0.0] * frames
    raw = []
    for window in windows:
        w = pyramid(len(window))
        slots = accumulate_slots(window)
        raw.append([(fr, float(wj)) for fr, wj in zip(slots, w)])
        for fr, wj in raw[-1]:
            if fr >= 0:
                total[fr] += wj
    return [[wj / total[fr] if fr >= 0 else 0.0 for fr, wj in row] for row in raw]
