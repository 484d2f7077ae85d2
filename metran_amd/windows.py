"""Time windows of ``MetranBatch.get_window_statistics`` and ``get_window_means``, translated to step ranges: a pure host function (pandas and numpy, no
engine).  Step ``t`` of model ``r`` is in the window ``(start, stop)`` when ``start <= index[r][t] < stop``; a model's steps are
those of its own index, so the padded steps beyond its length are in no window."""
import numpy as np

__all__ = ["step_windows"]


def _edges(index, alias):
    """The ticks of the offset ``alias`` from the last one at or before ``index[0]`` to the first one after ``index[-1]``."""
    from pandas import DatetimeIndex
    from pandas.tseries.frequencies import to_offset

    offset = to_offset(alias)
    edge = offset.rollback(index[0].normalize())
    edges = [edge]
    while edge <= index[-1]:
        edge = edge + offset
        edges.append(edge)
    return DatetimeIndex(edges)


def step_windows(indexes, windows, T, overlap=False):
    """``indexes``: one increasing ``DatetimeIndex`` per model (its length at most ``T``); ``windows``: a pandas offset alias
    (``"MS"``, ``"YS"``, ``"W"``, ...: the windows between consecutive ticks of the offset that cover the model's index) or a
    list of ``(start, stop)`` timestamps, sorted and not overlapping (``overlap=True``: in any order, overlapping or not -- the
    exact window means are computed window by window).  Returns ``(steps, starts)``: ``steps`` int64 ``[R,W,2]``
    half-open step ranges ``[a, b)`` per model -- a window without a step of the model is empty (``a == b``), models with fewer
    windows are padded with ``(T, T)`` -- and ``starts``, per model the ``DatetimeIndex`` of its windows' starts."""
    from pandas import DatetimeIndex, Timestamp

    T = int(T)
    spans = []
    for index in indexes:
        index = DatetimeIndex(index)
        if len(index) > T:
            raise ValueError("an index of %d steps is longer than T = %d" % (len(index), T))
        if len(index) == 0 or not index.is_monotonic_increasing:
            raise ValueError("every model needs a non-empty, increasing index")
        if isinstance(windows, str):
            edges = _edges(index, windows)
            start, stop = edges[:-1], edges[1:]
        else:
            pairs = [(Timestamp(a), Timestamp(b)) for a, b in windows]
            if not pairs:
                raise ValueError("windows is empty")
            start, stop = DatetimeIndex([p[0] for p in pairs]), DatetimeIndex([p[1] for p in pairs])
            if overlap and (stop < start).any():
                raise ValueError("every window needs start <= stop")
            if not overlap and ((stop < start).any() or (start[1:] < stop[:-1]).any()):
                raise ValueError("windows must be sorted and must not overlap: start <= stop <= the next window's start")
        spans.append((start, np.stack([index.searchsorted(start, side="left"), index.searchsorted(stop, side="left")], axis=1)))
    W = max(len(s[0]) for s in spans)
    steps = np.full((len(spans), W, 2), T, dtype=np.int64)
    for r, (_, ab) in enumerate(spans):
        steps[r, : len(ab)] = ab
    return steps, [s[0] for s in spans]
