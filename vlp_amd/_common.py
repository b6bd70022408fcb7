"""What the training engine (engine.py) and the caption decoder (decoder.py) both need, so that neither imports the other for it."""

PE_DIM = 1607         # 6 box numbers + 1601 class probabilities (modeling.py:1016)
PE_PAD = 1664         # next multiple of 64: GEMM K alignment


def _ru(x, m):
    return (x + m - 1) // m * m


class VlpPerformanceWarning(UserWarning):
    """A correct but avoidably slow way of driving the engine (issued once per engine)."""
