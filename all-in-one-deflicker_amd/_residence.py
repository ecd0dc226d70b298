"""Where the arrays of one handle-free library call live: numpy arrays handed over as host pointers (the library stages the call), or CUDA
tensors handed over as device pointers (nothing leaves the device).  The two classes are the two sides of one interface, so that an
operation's checks and its ctypes call are written once over a residence `res`:

    res.ordinal, res.on_device      the device ordinal and the flag the library takes
    res.array(x)                    x as this side's array type (numpy: np.asarray)
    res.typed(x, "uint8")           x lives on this side and has that dtype
    res.contiguous(x)               x made contiguous
    res.empty(shape, "uint8")       an output
    res.ptr(x)                      the pointer to pass to ctypes (None stays None)
    res.sync()                      what must happen between allocating and calling

torch is imported by the device side only."""
import ctypes as C

import numpy as np


class Host:
    on_device = 0

    def __init__(self, device=0):
        self.ordinal = int(device)

    def array(self, x):
        return np.asarray(x)

    def typed(self, x, dtype):
        return getattr(x, "dtype", None) == dtype      # a numpy dtype compares equal to its name

    def contiguous(self, x):
        return np.ascontiguousarray(x)

    def empty(self, shape, dtype):
        return np.empty(shape, np.dtype(dtype))

    def ptr(self, x):
        return None if x is None else x.ctypes.data_as(C.c_void_p)

    def sync(self):
        pass


class Device:
    on_device = 1

    def __init__(self, dev, ordinal=None, sync_current=False):
        """dev: the torch.device the tensors live on (outputs land there); ordinal: the device to name to the library when it is not dev's
        own; sync_current: synchronise torch's current device, not dev (resize_area_device has always done so)."""
        import torch
        self.torch, self.dev, self.sync_dev = torch, dev, None if sync_current else dev
        self.ordinal = dev.index if ordinal is None else int(ordinal)

    def array(self, x):
        return x

    def typed(self, x, dtype):
        return bool(getattr(x, "is_cuda", False)) and x.dtype == getattr(self.torch, dtype)

    def contiguous(self, x):
        return x.contiguous()

    def empty(self, shape, dtype):
        return self.torch.empty(tuple(shape), dtype=getattr(self.torch, dtype), device=self.dev)

    def ptr(self, x):
        return None if x is None else C.c_void_p(x.data_ptr())

    def sync(self):
        self.torch.cuda.synchronize(self.sync_dev)      # the tensors' producers ran on torch's streams, the library runs on the default one


def one_device(tensors, message):
    """The Device residence of CUDA tensors that all live on one device, or ValueError(message)."""
    dev = tensors[0].device if hasattr(tensors[0], "is_cuda") else None
    for t in tensors:
        if not hasattr(t, "is_cuda") or not t.is_cuda or t.device != dev:
            raise ValueError(message)
    return Device(dev)
