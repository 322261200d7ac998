"""The one timing loop of the benchmark scripts."""
import time

WINDOW = 20


def timed(fn, steps, warmup, torch, before_window=None, after_window=None, window=WINDOW):
    """Seconds per call of ``fn``: ``warmup`` untimed calls, then ``steps`` calls timed in windows of ``window`` with a ``torch.cuda.synchronize()``
    at both ends of each (the same for every leg of a comparison).  ``before_window`` / ``after_window`` run outside the timed region (untimed work
    that, say, re-initialises the world ``fn`` steps, or keeps one that ``fn`` only reads moving)."""
    for _ in range(warmup):
        fn()
    total, done = 0.0, 0
    while done < steps:
        w = min(window, steps - done)
        if before_window is not None:
            before_window()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(w):
            fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
        if after_window is not None:
            after_window()
        done += w
    return total / steps
