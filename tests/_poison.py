"""Scratch poison for tests: make uninitialised memory read as garbage instead of the zeros a fresh process usually sees.

Every byte of device memory the library touches comes from torch (there is no device allocation in csrc/), and most of it from
``torch.empty``.  A kernel that accumulates into memory nobody cleared, or reads a pad column nobody wrote, is wrong only when that
memory was not already zero -- which newly mapped device memory normally is.  The helpers here fill such memory with ``0xFF`` bytes:
NaN as float32 / float64 / bfloat16 / float16, -1 as a signed integer, 255 as uint8, True as bool.

  poison_(t)                 fill the bytes of one tensor
  poisoned_allocations()     context manager: ``torch.empty`` / ``torch.empty_like`` return poisoned memory (the two forms the package
                             calls; ``Tensor.new_empty`` and ``torch.empty_strided`` are not used by it)
  poison_buffers(obj, keep)  poison every tensor of an engine's buffer table except the names in ``keep``

The fills are ordinary torch ops on the current stream -- the stream the library's ``Context`` binds to -- so they are ordered with
the library's launches.  Never use ``poisoned_allocations`` around HIP-graph capture (the fill would be captured).

A plain module: no fixtures, no pytest settings."""
import contextlib

import torch

POISON_BYTE = 0xFF


def poison_(t):
    """fill every byte of ``t`` (any dtype, shape or stride; 0-dim and empty tensors included) with 0xFF, in place; returns ``t``"""
    if t.numel() == 0:
        return t
    if t.is_contiguous():
        t.view(-1).view(torch.uint8).fill_(POISON_BYTE)          # (a 0-dim tensor views as [1] first)
        return t
    # a strided view: only ITS elements (what lies between them belongs to somebody else)
    fill = torch.full((t.element_size(),), POISON_BYTE, dtype=torch.uint8, device=t.device).view(t.dtype)
    t.copy_(fill.reshape(()).expand(t.shape))
    return t


class PoisonCount:
    """what ``poisoned_allocations`` has filled so far"""

    def __init__(self):
        self.tensors = 0
        self.bytes = 0

    def __repr__(self):
        return "PoisonCount(tensors=%d, bytes=%d)" % (self.tensors, self.bytes)


@contextlib.contextmanager
def poisoned_allocations(devices=("cuda",)):
    """Inside the block ``torch.empty`` and ``torch.empty_like`` return memory filled with 0xFF when the result lies on a device
    whose type is in ``devices``.  Yields a ``PoisonCount``; the originals are back on exit, also after an exception."""
    devices = tuple(torch.device(d).type for d in devices)
    count = PoisonCount()
    originals = {"empty": torch.empty, "empty_like": torch.empty_like}

    def wrap(fn):
        def poisoned(*args, **kwargs):
            t = fn(*args, **kwargs)
            if isinstance(t, torch.Tensor) and t.device.type in devices:
                poison_(t)
                count.tensors += 1
                count.bytes += t.numel() * t.element_size()
            return t
        poisoned.__wrapped__ = fn
        return poisoned

    try:
        for name, fn in originals.items():
            setattr(torch, name, wrap(fn))
        yield count
    finally:
        for name, fn in originals.items():
            setattr(torch, name, fn)


def _walk(node, prefix, keep, done):
    if isinstance(node, torch.Tensor):
        if prefix in keep:
            return
        poison_(node)
        done.append(prefix)
    elif isinstance(node, dict):
        for k, v in node.items():
            name = k if isinstance(k, str) else repr(k)
            _walk(v, name if prefix is None else "%s/%s" % (prefix, name), keep, done)
    elif isinstance(node, (list, tuple)):
        for i, v in enumerate(node):
            _walk(v, "%s[%d]" % (prefix, i), keep, done)


def poison_buffers(mapping_or_obj, keep=()):
    """Poison every tensor of a buffer table -- a dict, or an object with a ``_buf`` dict -- except the names in ``keep``.  Nested
    dicts (the data-parallel ``wire / q_local / lbar_local`` set) are walked; their tensors are named ``outer/inner`` and an outer
    name in ``keep`` covers the whole nest.  Non-string keys are named by their ``repr``.  Returns the sorted names it poisoned."""
    table = mapping_or_obj if isinstance(mapping_or_obj, dict) else mapping_or_obj._buf
    keep = set(keep)
    done = []
    for k, v in table.items():
        name = k if isinstance(k, str) else repr(k)
        if name in keep:
            continue
        _walk(v, name, keep, done)
    return sorted(done)
