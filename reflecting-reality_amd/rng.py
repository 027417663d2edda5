"""Noise draws with the reference's generator semantics (utils/torch_utils.py randn_tensor): the draw happens on the
GENERATOR's device — a `torch.Generator('cuda')` (what examples/brushnet/test_brushnet.py:166 passes) draws on the GPU, a
CPU generator (or none) draws on the host and the result is uploaded; a list gives one generator per batch element.

PhiloxGenerator is the library's own stream (csrc/rng.hip; include/mfhip.h states it): counter-based, so a draw depends on (seed, offset)
alone — not on the grid, the device or the number of ranks — and a C host calling mf_philox_normal draws the same numbers."""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch


_M64 = (1 << 64) - 1


class PhiloxGenerator:
    """The pair (seed, offset) of the library's Philox4x32-10 stream, offset counted in blocks of four values.  Both are plain Python
    ints, advanced on the host by the documented counts (hip.philox_normal_blocks / philox_int_blocks), so reading them never touches
    the device.  Draws happen on `device` (default: the current cuda device) on the current stream.

    device_state() is the same pair in device memory, for a captured graph: draws given state= read it, hip.philox_advance moves it,
    and the host offset is advanced alongside (note_advanced), so it always equals what the device holds after the queued work."""

    def __init__(self, seed: int = 0, device: Union[None, str, torch.device] = None):
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[torch.Tensor] = None
        self._synced = None                 # the (seed, offset) the device state holds once the queued work has run
        self.manual_seed(seed)

    def manual_seed(self, seed: int) -> "PhiloxGenerator":
        return self.set_state((seed, 0))

    @property
    def seed(self) -> int:
        return self._seed

    @property
    def offset(self) -> int:
        return self._offset

    def get_state(self):
        return (self._seed, self._offset)

    def set_state(self, state) -> "PhiloxGenerator":
        seed, offset = state
        self._seed, self._offset = int(seed) & _M64, int(offset) & _M64
        return self

    def _device(self) -> torch.device:
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _upload(self) -> None:
        from . import hip
        self._state.copy_(torch.tensor([hip._s64(self._seed), hip._s64(self._offset)], dtype=torch.int64))
        self._synced = (self._seed, self._offset)

    def device_state(self) -> torch.Tensor:
        """int64 [2] on the device holding {seed, offset} as the library reads them (uint64).  Every call brings it level with the host
        pair (a copy only when eager draws or set_state moved the host pair since), so call it outside a graph capture."""
        if self._state is None:
            self._state = torch.empty(2, dtype=torch.int64, device=self._device())
        if self._synced != (self._seed, self._offset):
            self._upload()
        return self._state

    def note_advanced(self, blocks: int, on_device: bool = False) -> None:
        """The host pair moves by `blocks`; on_device: a queued hip.philox_advance moves the device state by the same count."""
        was = (self._seed, self._offset)
        self._offset = (self._offset + int(blocks)) & _M64
        if on_device and self._state is not None and self._synced == was:
            self._synced = (self._seed, self._offset)

    def device_moved(self) -> None:
        """Queued device work moved the device state and the host pair did NOT follow (a captured step that advances at a step whose
        update reads no noise): the next device_state() uploads the host pair again."""
        self._synced = None

    def randn(self, shape: Sequence[int], first_sample: int = 0, global_batch: Optional[int] = None, scale: float = 1.0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 normals [B, ...] drawn per sample: this call owns the samples [first_sample, first_sample + B) of a draw of
        global_batch (default first_sample + B); the offset advances by the WHOLE draw's blocks, as on every other rank."""
        from . import hip
        shape = tuple(int(d) for d in shape)
        g = shape[0] + first_sample if global_batch is None else int(global_batch)
        res = hip.philox_normal(shape, self._seed, self._offset, self._device(), scale, first_sample, g, out=out)
        per = 1
        for d in shape[1:]:
            per *= d
        self.note_advanced(hip.philox_normal_blocks(g, per))
        return res

    def randint(self, high: int, n: int, first: int = 0, total: Optional[int] = None) -> torch.Tensor:
        """int64 [n] below `high` (0 < high <= 2^31), the elements [first, first + n) of a draw of `total` (default first + n)."""
        from . import hip
        t = first + n if total is None else int(total)
        res = hip.philox_randint(high, n, self._seed, self._offset, self._device(), first, t)
        self.note_advanced(hip.philox_int_blocks(t))
        return res

    def bits(self, n: int) -> torch.Tensor:
        """n raw uint32 of the stream, as an int32 device tensor holding the bit patterns."""
        from . import hip
        res = hip.philox_bits(n, self._seed, self._offset, self._device())
        self.note_advanced(hip.philox_int_blocks(n))
        return res


def is_philox(generator) -> bool:
    if isinstance(generator, (list, tuple)):
        kinds = {isinstance(g, PhiloxGenerator) for g in generator}
        if kinds == {True, False}:
            raise ValueError("a list of generators is all PhiloxGenerator or all torch.Generator, not a mix")
        return kinds == {True}
    return isinstance(generator, PhiloxGenerator)


def randn_tensor(shape: Sequence[int], generator: Union[None, torch.Generator, List[torch.Generator], PhiloxGenerator,
                                                        List[PhiloxGenerator]] = None,
                 device: Union[None, str, torch.device] = None) -> torch.Tensor:
    shape = tuple(shape)
    device = torch.device(device) if device is not None else torch.device("cpu")
    if is_philox(generator):
        gens = list(generator) if isinstance(generator, (list, tuple)) else [generator]
        if len(gens) > 1 and len(gens) != shape[0]:
            raise ValueError(f"You have passed a list of generators of length {len(gens)}, but requested an effective batch size of "
                             f"{shape[0]}. Make sure the batch size matches the length of the generators.")
        if device.type != "cuda":
            raise ValueError(f"Cannot generate a {device} tensor from a PhiloxGenerator: it draws on the device")
        for g in gens:
            if g.device is None:
                g.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        if len(gens) == 1:
            return gens[0].randn(shape).to(device)
        return torch.cat([g.randn((1,) + shape[1:]).to(device) for g in gens], dim=0)
    if isinstance(generator, (list, tuple)):
        if len(generator) == 1:
            generator = generator[0]
        else:
            if len(generator) != shape[0]:
                raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an "
                                 f"effective batch size of {shape[0]}. Make sure the batch size matches the length of the "
                                 "generators.")
            return torch.cat([randn_tensor((1,) + shape[1:], g, device) for g in generator], dim=0)
    gdev = generator.device if generator is not None else torch.device("cpu")
    if gdev.type == "cuda" and device.type != "cuda":
        raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gdev.type}.")
    draw_on = gdev if generator is not None else torch.device("cpu")
    return torch.randn(shape, generator=generator, device=draw_on, dtype=torch.float32).to(device)
