"""Stream capture that no garbage collection can interrupt.

The loops' objects reference each other (a trainer, its model, the update plans and their launch
closures), so a dropped trainer is freed by the cyclic collector, whenever that next runs.  Its
finalisers free device memory (``aac_env_destroy`` calls hipFree) and release captured graphs, and a
stream capture forbids both: a collection that falls inside a capture breaks it.  torch collects ahead
of a capture only with ``torch.compiler.config.force_cudagraph_gc``.
"""
import contextlib
import gc

import torch


@contextlib.contextmanager
def capture(g, **kw):
    """``torch.cuda.graph(g, **kw)`` with the device drained and the dead cycles collected first, and the
    collector held off until the capture has ended."""
    torch.cuda.synchronize()
    gc.collect()
    on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kw):
            yield
    finally:
        if on:
            gc.enable()
