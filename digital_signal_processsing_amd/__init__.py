"""MI355X-native (gfx950) causal moving-average filter.

Host-side Python mirror of the reference's per-variant GPU drivers
(``<Variant>GpuLoad`` in ``basics/*.cu``): every call goes through the C ABI of
``libmavg.so`` (include/mavg.h) into hand-written HIP kernels.  PyTorch is used
only for device memory and streams.

    y = moving_average(x, grade=1024)                  # fp32 or int16 CUDA tensor
    y = moving_average(x, grade=32, channels=2, algo="hillis")
    y = moving_average_rows(x, grade=1024)             # [B, T] / [C, T] / [B, C, T]: every row on its own
    y = moving_average_ragged(x, grade=1024, lengths=[5, 0, 30011, 7])   # packed rows of different lengths
    y = moving_average_decimated(x, grade=400, hop=160)  # only every hop-th output frame, in one launch
    y = moving_rms(x, grade=1024)                      # fp32 RMS / variance / std of the window, one launch
    lo, hi = moving_minmax(x, grade=1024)              # the window's minimum and maximum (peak envelope), one launch
    y = exponential_moving_average(x, alpha=0.05)      # y[f] = (1-a) y[f-1] + a x[f], fp32 (or span= / halflife= / tau=)
    y = fir_filter(x, taps)                            # y[f] = sum_j taps[j] x[f-j], one fp64 fma chain per output, fp32

Semantics: ``basics/profilable_moving_averager.cpp:14-37`` -- interleaved
frames, window ``grade`` frames, zero history (or ``history``: the
(grade-1)*channels samples that precede ``x``), int16 output = exact
truncating ``S / grade``, fp32 output = ``S / grade`` with ``S`` in fp64.
"""
from __future__ import annotations

from typing import Optional

from . import _lib
from ._lib import (ALGOS, F32, FIR_AUTO, FIR_STRIP, FIR_TILE, I16, SOS_AUTO, SOS_LOOP, SOS_TILE, STATS, MavgError, MavgLibraryError,  # noqa: F401
                   algo_name, strerror)

__all__ = [
    "moving_average",
    "moving_average_into",
    "moving_average_rows",
    "moving_average_rows_into",
    "rows_plan",
    "rows_workspace_bytes",
    "moving_average_ragged",
    "moving_average_ragged_into",
    "ragged_plan",
    "ragged_workspace_bytes",
    "moving_average_decimated",
    "moving_average_decimated_into",
    "decim_out_frames",
    "decim_plan",
    "decim_workspace_bytes",
    "moving_average_cascade",
    "moving_average_cascade_into",
    "cascade_plan",
    "cascade_workspace_bytes",
    "moving_stat",
    "moving_stat_into",
    "moving_rms",
    "moving_variance",
    "moving_std",
    "moving_mean_square",
    "stat_plan",
    "STATS",
    "moving_max",
    "moving_min",
    "moving_minmax",
    "moving_extrema_into",
    "extrema_plan",
    "exponential_moving_average",
    "exponential_moving_average_into",
    "ema_alpha",
    "ema_plan",
    "ema_workspace_bytes",
    "ema_halo_frames",
    "biquad",
    "biquad_into",
    "biquad_plan",
    "biquad_workspace_bytes",
    "biquad_halo_frames",
    "sos_filter",
    "sosfilt",
    "sosfilt_into",
    "sos_plan",
    "sos_workspace_bytes",
    "sos_halo_frames",
    "fir_filter",
    "fir_filter_into",
    "fir_taps",
    "fir_plan",
    "fill_synthetic",
    "workspace_bytes",
    "resolve_algo",
    "plan",
    "stream_copy",
    "ALGOS",
    "MavgError",
    "MavgLibraryError",
]


def _torch():
    import torch
    return torch


def _dtype_code(t) -> int:
    torch = _torch()
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.int16:
        return I16
    raise TypeError(f"moving_average supports float32 and int16 tensors, got {t.dtype}")


def _algo_code(algo) -> int:
    if isinstance(algo, int):
        return algo
    try:
        return ALGOS[algo]
    except KeyError:
        raise ValueError(f"unknown algo {algo!r}; one of {sorted(ALGOS)}") from None


class _nullctx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def _stream_handle(stream, device) -> int:
    torch = _torch()
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return stream.cuda_stream


def _check_device_pair(x, out) -> None:
    if not (x.is_cuda and out.is_cuda):
        raise ValueError("x and out must be device tensors (libmavg has no CPU path)")
    if not (x.is_contiguous() and out.is_contiguous()):
        raise ValueError("x and out must be contiguous")


def _check_device_x(x) -> None:
    if not x.is_cuda:
        raise ValueError("x must be a device tensor (libmavg has no CPU path)")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")


def _history_ptr(history, x, samples: int, what: str):
    """The history's device pointer (None without one); it must hold ``samples`` = ``what`` samples."""
    if history is None:
        return None
    if history.dtype != x.dtype or not history.is_cuda or not history.is_contiguous():
        raise ValueError("history must be a contiguous device tensor of x's dtype")
    if history.numel() != samples:
        raise ValueError(f"history must hold {what} = {samples} samples")
    return history.data_ptr() if history.numel() else None


def _on_stream(stream, make):
    """``make()`` with the launch stream current: a block the caching allocator hands out there is
    free with respect to that stream's pending work (one taken on another stream could still be
    in use by kernels queued there, and record_stream only protects the free)."""
    torch = _torch()
    with torch.cuda.stream(stream) if stream is not None else _nullctx():
        return make()


def _check_workspace_tensor(workspace) -> int:
    """A caller's workspace tensor; its size in bytes."""
    if not (workspace.is_cuda and workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous device tensor")
    return workspace.numel() * workspace.element_size()


def _loop_workspace(ws_n: int, workspace, stream, device, query: str):
    """(workspace tensor or None, its bytes) for the per-row loops of the batch calls; ``query``
    names the function that tells the size."""
    torch = _torch()
    if not ws_n:
        return None, 0
    if workspace is not None:
        # (a workspace that is too small goes to the library: MAVG_ERR_WORKSPACE, nothing enqueued)
        return workspace, _check_workspace_tensor(workspace)
    if torch.cuda.is_current_stream_capturing():
        raise ValueError(f"this batch runs the per-row loop, which needs a {ws_n}-byte workspace: "
                         f"inside a graph capture pass workspace= (see {query}())")
    return _on_stream(stream, lambda: torch.empty(ws_n, dtype=torch.uint8, device=device)), ws_n


def _with_out(x, stream, into, inputs, shape=None):
    """``out = empty_like(x)`` (with ``shape``: that shape, ``x``'s dtype and device) filled by
    ``into(out)``.  On a launch stream other than the
    current one, the launch stream waits for the current one (where ``inputs`` come from),
    ``out`` is allocated on the launch stream, and the caching allocator is kept from handing
    the inputs' blocks out again before the kernel that reads them there ends."""
    torch = _torch()
    def make():
        return torch.empty_like(x) if shape is None else torch.empty(shape, dtype=x.dtype, device=x.device)

    if stream is None or stream == torch.cuda.current_stream(x.device):
        out = make()
        into(out)
        return out
    stream.wait_stream(torch.cuda.current_stream(x.device))
    out = _on_stream(stream, make)
    into(out)
    for t in inputs:
        if t is not None:
            t.record_stream(stream)
    return out


def workspace_bytes(n: int, grade: int, channels: int = 1, dtype: int = F32, algo="auto",
                    block_size: int = 0, library: Optional[str] = None) -> int:
    import ctypes
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_workspace_bytes(n, channels, grade, dtype, _algo_code(algo), block_size,
                                                ctypes.byref(out)), "mavg_workspace_bytes")
    return out.value


def resolve_algo(n: int, grade: int, channels: int = 1, dtype: int = F32, algo="auto",
                 library: Optional[str] = None) -> str:
    lib = _lib.load(library)
    return lib.mavg_algo_name(lib.mavg_resolve_algo(n, channels, grade, dtype, _algo_code(algo))).decode()


def plan(n: int, grade: int, channels: int = 1, dtype: int = F32, algo="auto", block_size: int = 0,
         library: Optional[str] = None) -> str:
    """The kernel and launch geometry mavg_run would use (nothing is launched)."""
    import ctypes
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load(library).mavg_plan(n, channels, grade, dtype, _algo_code(algo), block_size, buf, len(buf)),
               "mavg_plan")
    return buf.value.decode()


def moving_average_into(x, out, grade: int, channels: int = 1, algo="auto", history=None,
                        block_size: int = 0, stream=None, workspace=None, library: Optional[str] = None) -> None:
    """Enqueue ``out = moving_average(x)`` on ``stream`` (default: current).

    ``workspace``: optional caller-owned device buffer (any dtype, contiguous)
    of at least ``workspace_bytes(...)`` bytes, like the reference's
    ``DspWorkspace`` scratch; without it the look-back scan (long windows)
    takes one from torch's caching allocator per call.
    ``library``: path of another build of the same ABI (the debug build,
    ``_lib.DEBUG_LIB_PATH``); default the release ``libmavg.so``."""
    torch = _torch()
    _check_device_pair(x, out)
    if x.dtype != out.dtype or x.numel() != out.numel():
        raise ValueError("x and out must have the same dtype and size")
    dt = _dtype_code(x)
    hist_ptr = _history_ptr(history, x, (grade - 1) * channels, "(grade-1)*channels")
    # workspace (look-back scan only): from torch's caching allocator, tied to
    # the launch stream so it is not handed out again before the kernel ends
    ws_n = workspace_bytes(x.numel(), grade, channels, dt, algo, block_size, library)
    ws = None
    if ws_n and workspace is not None:
        have = _check_workspace_tensor(workspace)
        if have < ws_n:
            raise ValueError(f"workspace holds {have} bytes, the launch needs {ws_n}")
        ws, ws_n = workspace, have
    elif ws_n:
        if torch.cuda.is_current_stream_capturing():
            # a workspace taken from the capture's private pool is freed again
            # before the capture ends; pass one that outlives the graph
            raise ValueError(f"grade={grade} uses the look-back scan, which needs a {ws_n}-byte workspace: "
                             "inside a graph capture pass workspace= (see workspace_bytes())")
        ws = _on_stream(stream, lambda: torch.empty(ws_n, dtype=torch.uint8, device=x.device))
    st = _lib.load(library).mavg_run(x.data_ptr(), out.data_ptr(), x.numel(), channels, grade, dt,
                              _algo_code(algo), block_size, hist_ptr,
                              ws.data_ptr() if ws is not None else None, ws_n,
                              _stream_handle(stream, x.device))
    _lib.check(st, "mavg_run")


def moving_average(x, grade: int, channels: int = 1, algo="auto", history=None,
                   block_size: int = 0, stream=None, library: Optional[str] = None):
    """Causal ``grade``-frame moving average of an interleaved signal ``x``."""
    return _with_out(x, stream, lambda out: moving_average_into(x, out, grade, channels, algo, history, block_size,
                                                                stream, library=library), (x, history))


def rows_workspace_bytes(rows: int, row_frames: int, grade: int, channels: int = 1, dtype: int = F32,
                         with_history: bool = False, library: Optional[str] = None) -> int:
    """Device workspace ``moving_average_rows_into`` needs: 0 for the one-launch rows scan, the
    single-row requirement for the per-row loop."""
    import ctypes
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_rows_workspace_bytes(rows, row_frames, channels, grade, dtype,
                                                            1 if with_history else 0, ctypes.byref(out)),
               "mavg_rows_workspace_bytes")
    return out.value


def rows_plan(rows: int, row_frames: int, grade: int, channels: int = 1, dtype: int = F32,
              with_history: bool = False, library: Optional[str] = None) -> str:
    """What mavg_rows_run would do (nothing is launched): ``rows_scan<...> ... tile_frames=N ...``
    (one launch of the segmented rows scan) or ``rows_loop rows=R x <one row's plan>`` (one
    single-signal launch per row)."""
    import ctypes
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load(library).mavg_rows_plan(rows, row_frames, channels, grade, dtype, 1 if with_history else 0,
                                                 buf, len(buf)), "mavg_rows_plan")
    return buf.value.decode()


def _rows_shape(x, channels: int):
    """(rows, row_frames) of a batch tensor: with one channel the last dimension is time and all
    leading dimensions are rows ([C, T], [B, T], [B, C, T]); with ``channels`` > 1 the last
    dimension is the channel and the one before it is time ([B, T, C])."""
    if channels < 1:
        raise ValueError(f"channels must be >= 1, got {channels}")
    if channels == 1:
        if x.dim() < 1:
            raise ValueError("x must have a time dimension")
        row_frames = x.shape[-1]
    else:
        if x.dim() < 2 or x.shape[-1] != channels:
            raise ValueError(f"with channels={channels} x must be [..., time, {channels}], got {tuple(x.shape)}")
        row_frames = x.shape[-2]
    per_row = row_frames * channels
    return (x.numel() // per_row if per_row else 0), row_frames


def moving_average_rows_into(x, out, grade: int, channels: int = 1, history=None, stream=None, workspace=None,
                             library: Optional[str] = None) -> None:
    """Enqueue ``out = moving_average_rows(x)`` on ``stream`` (default: current).

    ``x``: a contiguous device batch of independent signals (see ``moving_average_rows``).
    ``history``: optional, ``rows * (grade-1) * channels`` samples, row r's history at
    ``r * (grade-1) * channels``.  ``workspace``: as in ``moving_average_into``; only the per-row
    loop needs one (``rows_workspace_bytes``), the one-launch rows scan needs none."""
    _check_device_pair(x, out)
    if x.dtype != out.dtype or x.shape != out.shape:
        raise ValueError("x and out must have the same dtype and shape")
    dt = _dtype_code(x)
    rows, row_frames = _rows_shape(x, channels)
    hist_ptr = _history_ptr(history, x, rows * (grade - 1) * channels, "rows*(grade-1)*channels")
    ws_n = rows_workspace_bytes(rows, row_frames, grade, channels, dt, hist_ptr is not None, library)
    ws, ws_n = _loop_workspace(ws_n, workspace, stream, x.device, "rows_workspace_bytes")
    st = _lib.load(library).mavg_rows_run(x.data_ptr(), out.data_ptr(), rows, row_frames, channels, grade, dt,
                                          hist_ptr, ws.data_ptr() if ws is not None else None, ws_n,
                                          _stream_handle(stream, x.device))
    _lib.check(st, "mavg_rows_run")


def moving_average_rows(x, grade: int, channels: int = 1, history=None, stream=None, library: Optional[str] = None):
    """Causal ``grade``-frame moving average of every row of a dense batch, each row filtered as
    ``moving_average`` would filter it alone (zero history before its first frame, divisor
    ``grade``), in one launch where the rows scan applies (``rows_plan``).

    ``channels == 1``: the last dimension is time, all leading dimensions are rows -- planar audio
    ``[C, T]``, batches ``[B, T]``, ``[B, C, T]``.  ``channels == C > 1``: ``[..., T, C]``,
    interleaved frames.  The output has ``x``'s shape."""
    _rows_shape(x, channels)
    _check_device_x(x)
    return _with_out(x, stream, lambda out: moving_average_rows_into(x, out, grade, channels, history, stream,
                                                                     library=library), (x, history))


def _host_offsets(offsets, lengths):
    """The rows + 1 frame offsets as a contiguous host int64 tensor, from exactly one of
    ``offsets`` (rows + 1 entries) or ``lengths`` (rows entries, cumulated here); either a host
    int64 tensor, a sequence or a numpy array."""
    torch = _torch()
    if (offsets is None) == (lengths is None):
        raise ValueError("give exactly one of offsets= and lengths=")
    given = offsets if offsets is not None else lengths
    what = "offsets" if offsets is not None else "lengths"
    if isinstance(given, torch.Tensor) and given.is_cuda:
        raise ValueError(f"{what} must be in host memory (the device copy goes in offsets_device=)")
    try:
        t = torch.as_tensor(given)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{what} must be a host int64 tensor, a sequence or a numpy array of integers: {e}") from None
    if t.numel() and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool):
        raise ValueError(f"{what} must be integers, got {t.dtype}")
    t = t.to(torch.int64)
    if t.dim() != 1:
        raise ValueError(f"{what} must be one-dimensional, got shape {tuple(t.shape)}")
    if lengths is not None:
        if t.numel() and int(t.min()) < 0:
            raise ValueError("lengths must be >= 0")
        off = torch.zeros(t.numel() + 1, dtype=torch.int64)
        torch.cumsum(t, 0, out=off[1:])
        return off
    if t.numel() < 1:
        raise ValueError("offsets must hold rows + 1 entries (at least the leading 0)")
    if int(t[0]) != 0:
        raise ValueError(f"offsets must start at 0, got {int(t[0])}")
    if t.numel() > 1 and bool((t[1:] < t[:-1]).any()):
        raise ValueError("offsets must be non-decreasing")
    return t.contiguous()


def _offsets_ptr(off):
    import ctypes
    return ctypes.cast(off.data_ptr(), ctypes.POINTER(ctypes.c_int64))


def ragged_workspace_bytes(offsets, grade: int, channels: int = 1, dtype: int = F32,
                           library: Optional[str] = None) -> int:
    """Device workspace ``moving_average_ragged_into`` needs: 0 for the one-launch ragged scan,
    the longest row's single-signal requirement for the per-row loop."""
    import ctypes
    off = _host_offsets(offsets, None)
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_ragged_workspace_bytes(_offsets_ptr(off), off.numel() - 1, channels, grade,
                                                              dtype, ctypes.byref(out)), "mavg_ragged_workspace_bytes")
    return out.value


def ragged_plan(offsets, grade: int, channels: int = 1, dtype: int = F32, library: Optional[str] = None) -> str:
    """What mavg_ragged_run would do (nothing is launched): ``ragged_scan<...> rows=R frames=N
    max_row_frames=M window=min(grade,M) ... tile_frames=T ...`` (one launch of the ragged scan) or
    ``ragged_loop rows=R max_row_frames=M x <the longest row's plan>`` (one single-signal launch
    per non-empty row)."""
    import ctypes
    off = _host_offsets(offsets, None)
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load(library).mavg_ragged_plan(_offsets_ptr(off), off.numel() - 1, channels, grade, dtype,
                                                   buf, len(buf)), "mavg_ragged_plan")
    return buf.value.decode()


def _ragged_frames(x, channels: int) -> int:
    """Frames of a packed ragged batch: ``[frames]`` with one channel, ``[frames, C]`` interleaved."""
    if channels < 1:
        raise ValueError(f"channels must be >= 1, got {channels}")
    if channels == 1:
        if x.dim() != 1:
            raise ValueError(f"with channels=1 x must be the packed stream [frames], got {tuple(x.shape)}")
    elif x.dim() != 2 or x.shape[-1] != channels:
        raise ValueError(f"with channels={channels} x must be [frames, {channels}], got {tuple(x.shape)}")
    return x.shape[0]


def moving_average_ragged_into(x, out, grade: int, offsets=None, lengths=None, channels: int = 1,
                               offsets_device=None, stream=None, workspace=None,
                               library: Optional[str] = None) -> None:
    """Enqueue ``out = moving_average_ragged(x)`` on ``stream`` (default: current).

    ``x``: the packed device tensor, ``[frames]`` (one channel) or ``[frames, C]`` interleaved;
    row r is frames ``offsets[r] .. offsets[r+1]``.  Exactly one of ``offsets`` (rows + 1 entries,
    starting at 0, non-decreasing, ending at x's frame count) or ``lengths`` (rows entries,
    cumulated on the host): a host int64 tensor, a sequence or a numpy array.
    ``offsets_device``: optional int64 device tensor holding the same rows + 1 offsets (what the
    kernel reads); without it the offsets are uploaded on the launch stream, which a graph
    capture cannot do -- pass it there.  ``workspace``: as in ``moving_average_rows_into``; only
    the per-row loop needs one (``ragged_workspace_bytes``)."""
    torch = _torch()
    _check_device_pair(x, out)
    if x.dtype != out.dtype or x.shape != out.shape:
        raise ValueError("x and out must have the same dtype and shape")
    dt = _dtype_code(x)
    frames = _ragged_frames(x, channels)
    off = _host_offsets(offsets, lengths)
    rows = off.numel() - 1
    if int(off[-1]) != frames:
        raise ValueError(f"the offsets end at {int(off[-1])} frames, x holds {frames}")
    if offsets_device is not None:
        if not (offsets_device.is_cuda and offsets_device.is_contiguous() and offsets_device.dtype == torch.int64):
            raise ValueError("offsets_device must be a contiguous int64 device tensor")
        if offsets_device.numel() != rows + 1:
            raise ValueError(f"offsets_device must hold rows + 1 = {rows + 1} entries, got {offsets_device.numel()}")
    ws_n = ragged_workspace_bytes(off, grade, channels, dt, library)
    if rows == 0 or frames == 0:
        return  # validated above and by the library's workspace query; nothing to enqueue
    if offsets_device is None:
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("the offsets would be uploaded to the device here: inside a graph capture pass "
                             "offsets_device= (an int64 device tensor of the rows + 1 offsets)")
        # on the launch stream itself (a copy from pageable host memory returns when it is staged)
        offsets_device = _on_stream(stream, lambda: off.to(x.device))
    ws, ws_n = _loop_workspace(ws_n, workspace, stream, x.device, "ragged_workspace_bytes")
    st = _lib.load(library).mavg_ragged_run(x.data_ptr(), out.data_ptr(), _offsets_ptr(off),
                                            offsets_device.data_ptr(), rows, channels, grade, dt,
                                            ws.data_ptr() if ws is not None else None, ws_n,
                                            _stream_handle(stream, x.device))
    _lib.check(st, "mavg_ragged_run")
    if stream is not None:
        offsets_device.record_stream(stream)


def moving_average_ragged(x, grade: int, offsets=None, lengths=None, channels: int = 1, offsets_device=None,
                          stream=None, library: Optional[str] = None):
    """Causal ``grade``-frame moving average of every row of a packed ragged batch, each row
    filtered as ``moving_average`` would filter it alone (zero history before its first frame,
    divisor ``grade``), in one launch where the ragged scan applies (``ragged_plan``).  Arguments
    as ``moving_average_ragged_into``; the output has ``x``'s shape."""
    _ragged_frames(x, channels)
    _check_device_x(x)
    return _with_out(x, stream, lambda out: moving_average_ragged_into(x, out, grade, offsets, lengths, channels,
                                                                       offsets_device, stream, library=library), (x,))


def _check_hop_phase(hop: int, phase: int) -> None:
    if hop < 1:
        raise ValueError(f"hop must be >= 1, got {hop}")
    if not 0 <= phase < hop:
        raise ValueError(f"phase must be in [0, hop) = [0, {hop}), got {phase}")


def decim_out_frames(n_frames: int, hop: int, phase: int = 0, library: Optional[str] = None) -> int:
    """``len(range(phase, n_frames, hop))``: the frames ``moving_average_decimated`` returns."""
    import ctypes
    _check_hop_phase(hop, phase)
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_decim_out_frames(n_frames, hop, phase, ctypes.byref(out)), "mavg_decim_out_frames")
    return out.value


def decim_workspace_bytes(n: int, grade: int, hop: int, phase: int = 0, channels: int = 1, dtype: int = F32,
                          library: Optional[str] = None) -> int:
    """Device workspace ``moving_average_decimated_into`` needs: 0 for the one-launch paths
    (``decim_scan``, ``decim_window``), the full-rate output plus ``workspace_bytes`` for
    ``decim_full``, ``workspace_bytes`` for ``hop == 1``."""
    import ctypes
    _check_hop_phase(hop, phase)
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_decim_workspace_bytes(n, channels, grade, hop, phase, dtype, ctypes.byref(out)),
               "mavg_decim_workspace_bytes")
    return out.value


def decim_plan(n: int, grade: int, hop: int, phase: int = 0, channels: int = 1, dtype: int = F32,
               library: Optional[str] = None) -> str:
    """What mavg_decim_run would do (nothing is launched): ``decim_none x <plan>``,
    ``decim_window<...> ...``, ``decim_scan<...> ... tile_frames=N ...`` or
    ``decim_full hop=H phase=P x <plan>``."""
    import ctypes
    _check_hop_phase(hop, phase)
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load(library).mavg_decim_plan(n, channels, grade, hop, phase, dtype, buf, len(buf)), "mavg_decim_plan")
    return buf.value.decode()


def _decim_shape(x, channels: int):
    """(frames, channels) of a signal for the decimated calls: ``[n]`` interleaved samples with
    ``channels`` channels, or ``[frames, C]``."""
    if channels < 1:
        raise ValueError(f"channels must be >= 1, got {channels}")
    if x.dim() == 1:
        if x.shape[0] % channels:
            raise ValueError(f"x holds {x.shape[0]} samples, not a multiple of channels={channels}")
        return x.shape[0] // channels, channels
    if x.dim() == 2:
        if channels not in (1, x.shape[1]):
            raise ValueError(f"with channels={channels} a 2-D x must be [frames, {channels}], got {tuple(x.shape)}")
        return x.shape[0], x.shape[1]
    raise ValueError(f"x must be [samples] or [frames, channels], got {tuple(x.shape)}")


def moving_average_decimated_into(x, out, grade: int, hop: int, phase: int = 0, channels: int = 1, history=None,
                                  stream=None, workspace=None, library: Optional[str] = None) -> None:
    """Enqueue ``out = moving_average_decimated(x)`` on ``stream`` (default: current).

    ``out``: a contiguous device tensor of ``decim_out_frames(frames, hop, phase) * channels``
    samples.  ``workspace``: as in ``moving_average_rows_into``; only the full-rate fallback (and
    ``hop == 1`` at long windows) needs one (``decim_workspace_bytes``)."""
    _check_hop_phase(hop, phase)
    frames, C = _decim_shape(x, channels)
    if x.dtype != out.dtype:
        raise ValueError("x and out must have the same dtype")
    M = len(range(phase, frames, hop))
    if out.numel() != M * C:
        raise ValueError(f"out must hold out_frames * channels = {M} * {C} samples, got {out.numel()}")
    _check_device_pair(x, out)
    dt = _dtype_code(x)
    hist_ptr = _history_ptr(history, x, (grade - 1) * C, "(grade-1)*channels")
    ws_n = decim_workspace_bytes(x.numel(), grade, hop, phase, C, dt, library)
    ws, ws_n = _loop_workspace(ws_n, workspace, stream, x.device, "decim_workspace_bytes")
    st = _lib.load(library).mavg_decim_run(x.data_ptr(), out.data_ptr(), x.numel(), C, grade, hop, phase, dt, hist_ptr,
                                           ws.data_ptr() if ws is not None else None, ws_n,
                                           _stream_handle(stream, x.device))
    _lib.check(st, "mavg_decim_run")


def moving_average_decimated(x, grade: int, hop: int, phase: int = 0, channels: int = 1, history=None, stream=None,
                             library: Optional[str] = None):
    """Frames ``phase, phase + hop, ...`` of ``moving_average(x, grade)`` -- what
    ``moving_average(x).view(-1, C)[phase::hop]`` gives -- without writing (or, for windows no
    longer than the hop, reading) what is dropped; one launch where ``decim_plan`` says
    ``decim_scan`` or ``decim_window``.  ``x``: ``[n]`` interleaved samples -> ``[M * channels]``,
    or ``[frames, C]`` -> ``[M, C]``."""
    _check_device_x(x)
    _check_hop_phase(hop, phase)
    frames, C = _decim_shape(x, channels)
    M = len(range(phase, frames, hop))
    shape = (M * C,) if x.dim() == 1 else (M, C)
    return _with_out(x, stream, lambda out: moving_average_decimated_into(x, out, grade, hop, phase, C, history, stream,
                                                                          library=library), (x, history), shape)


def _check_passes(passes: int) -> None:
    if passes < 1:
        raise ValueError(f"passes must be >= 1, got {passes}")


def cascade_workspace_bytes(n: int, grade: int, passes: int, channels: int = 1, dtype: int = F32,
                            with_history: bool = False, library: Optional[str] = None) -> int:
    """Device workspace ``moving_average_cascade_into`` needs: 0 for the one-launch fused kernel
    (``cascade_tile``), ``workspace_bytes`` for ``passes == 1``, and for ``cascade_loop`` the
    ping-pong buffer, with a history two history-block buffers, plus ``workspace_bytes``."""
    import ctypes
    _check_passes(passes)
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_cascade_workspace_bytes(n, channels, grade, passes, dtype, int(bool(with_history)),
                                                               ctypes.byref(out)), "mavg_cascade_workspace_bytes")
    return out.value


def cascade_plan(n: int, grade: int, passes: int, channels: int = 1, dtype: int = F32, with_history: bool = False,
                 library: Optional[str] = None) -> str:
    """What mavg_cascade_run would do (nothing is launched): ``cascade_none x <plan>``,
    ``cascade_tile<...> ... tile_frames=N ...`` or ``cascade_loop passes=P history=0|1 x <plan>``."""
    import ctypes
    _check_passes(passes)
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load(library).mavg_cascade_plan(n, channels, grade, passes, dtype, int(bool(with_history)), buf,
                                                    len(buf)), "mavg_cascade_plan")
    return buf.value.decode()


def moving_average_cascade_into(x, out, grade: int, passes: int, channels: int = 1, history=None, stream=None,
                                workspace=None, library: Optional[str] = None) -> None:
    """Enqueue ``out = moving_average_cascade(x)`` on ``stream`` (default: current).

    ``out``: a contiguous device tensor of ``x``'s size that does not overlap ``x``.  ``history``:
    the ``passes * (grade-1) * channels`` samples in front of ``x``.  ``workspace``: as in
    ``moving_average_rows_into``; only the loop (and ``passes == 1`` at long windows) needs one
    (``cascade_workspace_bytes``)."""
    _check_passes(passes)
    frames, C = _decim_shape(x, channels)
    if x.dtype != out.dtype:
        raise ValueError("x and out must have the same dtype")
    if out.numel() != x.numel():
        raise ValueError(f"out must hold x's {x.numel()} samples, got {out.numel()}")
    _check_device_pair(x, out)
    dt = _dtype_code(x)
    hist_ptr = _history_ptr(history, x, passes * (grade - 1) * C, "passes*(grade-1)*channels")
    ws_n = cascade_workspace_bytes(x.numel(), grade, passes, C, dt, history is not None, library)
    ws, ws_n = _loop_workspace(ws_n, workspace, stream, x.device, "cascade_workspace_bytes")
    st = _lib.load(library).mavg_cascade_run(x.data_ptr(), out.data_ptr(), x.numel(), C, grade, passes, dt, hist_ptr,
                                             ws.data_ptr() if ws is not None else None, ws_n,
                                             _stream_handle(stream, x.device))
    _lib.check(st, "mavg_cascade_run")


def moving_average_cascade(x, grade: int, passes: int, channels: int = 1, history=None, stream=None,
                           library: Optional[str] = None):
    """``passes`` successive ``moving_average(x, grade)`` passes with zero history (two: a
    triangular window; three or four: the usual Gaussian approximation), the intermediate kept in
    ``x``'s dtype; one launch where ``cascade_plan`` says ``cascade_tile``.  ``x``: ``[n]``
    interleaved samples or ``[frames, C]``; the result has ``x``'s shape."""
    _check_device_x(x)
    _check_passes(passes)
    _decim_shape(x, channels)
    C = channels if x.dim() == 1 else x.shape[1]
    return _with_out(x, stream, lambda out: moving_average_cascade_into(x, out, grade, passes, C, history, stream,
                                                                        library=library), (x, history))


def _stat_code(stat) -> int:
    if isinstance(stat, bool):
        raise ValueError(f"unknown stat {stat!r}; one of {sorted(STATS)} or 0..3")
    if isinstance(stat, int):
        if stat not in STATS.values():
            raise ValueError(f"unknown stat {stat!r}; one of {sorted(STATS)} or 0..3")
        return stat
    try:
        return STATS[stat]
    except (KeyError, TypeError):
        raise ValueError(f"unknown stat {stat!r}; one of {sorted(STATS)} or 0..3") from None


def stat_plan(n: int, grade: int, stat, channels: int = 1, dtype: int = F32, with_mean: bool = False,
              library: Optional[str] = None) -> str:
    """What mavg_stat_run would do (nothing is launched): ``stat_tile<...> ... tile_frames=N ...``
    or ``stat_strip ... L=...``."""
    import ctypes
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load(library).mavg_stat_plan(n, channels, grade, _stat_code(stat), dtype, int(bool(with_mean)), buf,
                                                 len(buf)), "mavg_stat_plan")
    return buf.value.decode()


def moving_stat_into(x, out, grade: int, stat, channels: int = 1, history=None, mean_out=None, stream=None,
                     library: Optional[str] = None) -> None:
    """Enqueue ``out = moving_stat(x)`` on ``stream`` (default: current), one launch, no workspace.

    ``out`` (and ``mean_out``, which receives the window mean): contiguous ``float32`` device
    tensors of ``x``'s size that do not overlap ``x``.  ``history``: the ``(grade-1) * channels``
    samples in front of ``x``."""
    torch = _torch()
    code = _stat_code(stat)
    frames, C = _decim_shape(x, channels)
    dt = _dtype_code(x)
    for t, what in ((out, "out"), (mean_out, "mean_out")):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise ValueError(f"{what} must be float32 (the statistics are fp32 for every input dtype), got {t.dtype}")
        if t.numel() != x.numel():
            raise ValueError(f"{what} must hold x's {x.numel()} samples, got {t.numel()}")
    _check_device_pair(x, out)
    if mean_out is not None:
        _check_device_pair(x, mean_out)
    hist_ptr = _history_ptr(history, x, (grade - 1) * C, "(grade-1)*channels")
    st = _lib.load(library).mavg_stat_run(x.data_ptr(), out.data_ptr(),
                                          mean_out.data_ptr() if mean_out is not None else None, x.numel(), C, grade,
                                          code, dt, hist_ptr, _stream_handle(stream, x.device))
    _lib.check(st, "mavg_stat_run")


def moving_stat(x, grade: int, stat, channels: int = 1, history=None, with_mean: bool = False, stream=None,
                library: Optional[str] = None):
    """A statistic of the causal ``grade``-frame window of ``x`` (fp32 or int16), per channel, as
    ``float32`` in ``x``'s shape: ``stat`` = ``"meansq"`` (S2/k), ``"rms"``, ``"var"`` (population
    variance, clamped at 0) or ``"std"`` -- or the ``mavg_stat`` value.  The divisor is ``grade``
    everywhere (the warm-up sees a zero-padded window, or ``history``).  ``with_mean``: return
    ``(y, mean)``, the window mean from the same launch.  fp32 variance is accurate to 1e-5 of the
    window's mean SQUARE: remove a large DC offset first."""
    torch = _torch()
    _check_device_x(x)
    _stat_code(stat)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    like = x.new_empty(0, dtype=torch.float32)  # _with_out's model: x's device, float32
    mean = []

    def into(out):
        if with_mean:
            mean.append(_on_stream(stream, lambda: torch.empty_like(out)))
        moving_stat_into(x, out, grade, stat, C, history, mean[0] if mean else None, stream, library)

    out = _with_out(like, stream, into, (x, history), tuple(x.shape))
    return (out, mean[0]) if with_mean else out


def moving_mean_square(x, grade: int, channels: int = 1, **kw):
    """``moving_stat(x, grade, "meansq", ...)``: the window's mean square S2/k."""
    return moving_stat(x, grade, "meansq", channels, **kw)


def moving_rms(x, grade: int, channels: int = 1, **kw):
    """``moving_stat(x, grade, "rms", ...)``: the window's root mean square."""
    return moving_stat(x, grade, "rms", channels, **kw)


def moving_variance(x, grade: int, channels: int = 1, **kw):
    """``moving_stat(x, grade, "var", ...)``: the window's population variance."""
    return moving_stat(x, grade, "var", channels, **kw)


def moving_std(x, grade: int, channels: int = 1, **kw):
    """``moving_stat(x, grade, "std", ...)``: the window's population standard deviation."""
    return moving_stat(x, grade, "std", channels, **kw)


def extrema_plan(n: int, grade: int, channels: int = 1, dtype: int = F32, with_max: bool = True, with_min: bool = True,
                 library: Optional[str] = None, aligned: bool = True) -> str:
    """What mavg_extrema_run would do (nothing is launched): ``extrema_tile<...> ... tile_frames=N ...``
    or ``extrema_strip ... L=...``.  ``aligned=False``: for views off 16-B alignment (the frame-unit
    form, ``F=1``)."""
    import ctypes
    buf = ctypes.create_string_buffer(512)
    given = 1 if aligned else 3    # bit 1: views off 16-B alignment
    _lib.check(_lib.load(library).mavg_extrema_plan(n, channels, grade, dtype, given if with_max else 0,
                                                    given if with_min else 0, buf, len(buf)), "mavg_extrema_plan")
    return buf.value.decode()


def moving_extrema_into(x, max_out, min_out, grade: int, channels: int = 1, history=None, stream=None,
                        library: Optional[str] = None) -> None:
    """Enqueue the moving maximum and / or minimum of ``x`` on ``stream`` (default: current), one
    launch, no workspace.

    ``max_out`` and ``min_out``: contiguous device tensors of ``x``'s dtype and size that overlap
    neither ``x`` nor each other; either may be ``None``, not both.  ``history``: the
    ``(grade-1) * channels`` samples in front of ``x``; without one the window is truncated at
    frame 0 (pass zeros for zero padding)."""
    frames, C = _decim_shape(x, channels)
    dt = _dtype_code(x)
    if max_out is None and min_out is None:
        raise ValueError("max_out and min_out must not both be None")
    for t, what in ((max_out, "max_out"), (min_out, "min_out")):
        if t is None:
            continue
        if t.dtype != x.dtype:
            raise ValueError(f"{what} must have x's dtype {x.dtype} (an extremum is one of the samples), got {t.dtype}")
        if t.numel() != x.numel():
            raise ValueError(f"{what} must hold x's {x.numel()} samples, got {t.numel()}")
    for t in (max_out, min_out):
        if t is not None:
            _check_device_pair(x, t)
    hist_ptr = _history_ptr(history, x, (grade - 1) * C, "(grade-1)*channels")
    st = _lib.load(library).mavg_extrema_run(x.data_ptr(), max_out.data_ptr() if max_out is not None else None,
                                             min_out.data_ptr() if min_out is not None else None, x.numel(), C, grade,
                                             dt, hist_ptr, _stream_handle(stream, x.device))
    _lib.check(st, "mavg_extrema_run")


def _moving_extrema(x, grade: int, channels: int, history, stream, library, want_max: bool, want_min: bool):
    torch = _torch()
    _check_device_x(x)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    second = []

    def into(out):
        if want_max and want_min:
            second.append(_on_stream(stream, lambda: torch.empty_like(out)))
            moving_extrema_into(x, second[0], out, grade, C, history, stream, library)
        elif want_max:
            moving_extrema_into(x, out, None, grade, C, history, stream, library)
        else:
            moving_extrema_into(x, None, out, grade, C, history, stream, library)

    out = _with_out(x, stream, into, (x, history))
    return (out, second[0]) if second else out


def moving_max(x, grade: int, channels: int = 1, history=None, stream=None, library: Optional[str] = None):
    """Per channel the largest sample of the causal ``grade``-frame window of ``x`` (fp32 or int16),
    in ``x``'s dtype and shape: a peak envelope, ``rolling(grade).max()``, a 1-D dilation.  Without
    ``history`` the window is truncated at frame 0."""
    return _moving_extrema(x, grade, channels, history, stream, library, True, False)


def moving_min(x, grade: int, channels: int = 1, history=None, stream=None, library: Optional[str] = None):
    """Per channel the smallest sample of the causal ``grade``-frame window of ``x``; see ``moving_max``."""
    return _moving_extrema(x, grade, channels, history, stream, library, False, True)


def moving_minmax(x, grade: int, channels: int = 1, history=None, stream=None, library: Optional[str] = None):
    """``(min, max)`` of the causal ``grade``-frame window from one launch and one read of ``x``
    (peak-to-peak is ``max - min``; the absolute peak ``maximum(max, -min)``)."""
    return _moving_extrema(x, grade, channels, history, stream, library, True, True)


def ema_alpha(alpha=None, span=None, halflife=None, tau=None) -> float:
    """The EMA coefficient from exactly one of ``alpha``, ``span`` (``2 / (span + 1)``),
    ``halflife`` (``1 - 2**(-1/halflife)``) or ``tau`` (``1 - exp(-1/tau)``), the last three in
    frames."""
    import math
    given = [(n, v) for n, v in (("alpha", alpha), ("span", span), ("halflife", halflife), ("tau", tau)) if v is not None]
    if len(given) != 1:
        raise ValueError("exactly one of alpha, span, halflife and tau must be given, got "
                         + (", ".join(n for n, _ in given) or "none"))
    name, v = given[0]
    v = float(v)
    if name == "alpha":
        a = v
    elif name == "span":
        if not v >= 1:
            raise ValueError(f"span must be >= 1, got {v}")
        a = 2.0 / (v + 1.0)
    else:
        if not v > 0:
            raise ValueError(f"{name} must be > 0, got {v}")
        a = -math.expm1(-math.log(2.0) / v) if name == "halflife" else -math.expm1(-1.0 / v)
    if not (math.isfinite(a) and 0.0 < a <= 1.0):
        raise ValueError(f"the coefficient must lie in (0, 1], got {a} from {name}={v}")
    return a


def ema_halo_frames(alpha: float, library: Optional[str] = None) -> int:
    """``H``: the smallest ``H >= 0`` with ``(1 - alpha)**H <= 2**-30`` -- how far back ``ema_tile``
    reads to rebuild a tile's carry."""
    import ctypes
    out = ctypes.c_longlong(0)
    _lib.check(_lib.load(library).mavg_ema_halo_frames(alpha, ctypes.byref(out)), "mavg_ema_halo_frames")
    return out.value


def ema_workspace_bytes(n: int, alpha: float, channels: int = 1, dtype: int = F32, library: Optional[str] = None) -> int:
    """Device workspace ``exponential_moving_average_into`` needs: 0 for ``ema_tile``, one fp64
    record per 1024-frame tile (``ema_chain``) or per strip (``ema_strip``) and channel."""
    import ctypes
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_ema_workspace_bytes(n, channels, alpha, dtype, ctypes.byref(out)),
               "mavg_ema_workspace_bytes")
    return out.value


def ema_plan(n: int, alpha: float, channels: int = 1, dtype: int = F32, state: bool = False, return_state: bool = False,
             library: Optional[str] = None, aligned: bool = True) -> str:
    """What mavg_ema_run would do (nothing is launched): ``ema_tile<...> ... halo_frames=H ...
    tile_frames=N ...``, ``ema_chain<...> ... records=R carry_chunk=K launches=3`` or ``ema_strip
    ... L=...``.  ``aligned=False``: for views off 16-B alignment (the frame-unit form, ``F=1``)."""
    import ctypes
    buf = ctypes.create_string_buffer(512)
    flags = (1 if state else 0) | (2 if return_state else 0) | (0 if aligned else 4)
    _lib.check(_lib.load(library).mavg_ema_plan(n, channels, alpha, dtype, flags, buf, len(buf)), "mavg_ema_plan")
    return buf.value.decode()


def _ema_state_ptr(state, C: int, what: str):
    torch = _torch()
    if state is None:
        return None
    if state.dtype != torch.float64:
        raise ValueError(f"{what} must be float64 (the carry is kept in fp64), got {state.dtype}")
    if state.numel() != C:
        raise ValueError(f"{what} must hold channels = {C} values, got {state.numel()}")
    if not state.is_cuda or not state.is_contiguous():
        raise ValueError(f"{what} must be a contiguous device tensor")
    return state.data_ptr()


def exponential_moving_average_into(x, out, alpha=None, *, span=None, halflife=None, tau=None, channels: int = 1,
                                    state=None, state_out=None, stream=None, workspace=None,
                                    library: Optional[str] = None) -> None:
    """Enqueue ``out = exponential_moving_average(x)`` on ``stream`` (default: current).

    ``out``: a contiguous ``float32`` device tensor of ``x``'s size that does not overlap ``x``.
    ``state`` / ``state_out``: ``float64`` device tensors of ``channels`` values -- ``y[-1]``, and
    where ``y[last frame]`` goes; not the same tensor.  ``workspace``: as in
    ``moving_average_rows_into``; ``ema_chain`` and ``ema_strip`` need one (``ema_workspace_bytes``)."""
    torch = _torch()
    a = ema_alpha(alpha, span, halflife, tau)
    frames, C = _decim_shape(x, channels)
    dt = _dtype_code(x)
    if out.dtype != torch.float32:
        raise ValueError(f"out must be float32 (the EMA is fp32 for every input dtype), got {out.dtype}")
    if out.numel() != x.numel():
        raise ValueError(f"out must hold x's {x.numel()} samples, got {out.numel()}")
    for t, what in ((state, "state"), (state_out, "state_out")):
        if t is not None and (t.dtype != torch.float64 or t.numel() != C):
            raise ValueError(f"{what} must be a float64 tensor of channels = {C} values, got {t.dtype} x {t.numel()}")
    _check_device_pair(x, out)
    sin = _ema_state_ptr(state, C, "state")
    sout = _ema_state_ptr(state_out, C, "state_out")
    if sin is not None and sin == sout:
        raise ValueError("state and state_out must not be the same tensor")
    ws_n = ema_workspace_bytes(x.numel(), a, C, dt, library)
    ws, ws_n = _loop_workspace(ws_n, workspace, stream, x.device, "ema_workspace_bytes")
    st = _lib.load(library).mavg_ema_run(x.data_ptr(), out.data_ptr(), x.numel(), C, a, dt, sin, sout,
                                         ws.data_ptr() if ws is not None else None, ws_n,
                                         _stream_handle(stream, x.device))
    _lib.check(st, "mavg_ema_run")


def exponential_moving_average(x, alpha=None, *, span=None, halflife=None, tau=None, channels: int = 1, state=None,
                               return_state: bool = False, stream=None, workspace=None,
                               library: Optional[str] = None):
    """``y[f] = (1 - alpha) y[f-1] + alpha x[f]`` per channel of ``x`` (fp32 or int16), as
    ``float32`` in ``x``'s shape: ``ewm(adjust=False).mean()``, a one-pole low-pass.  Exactly one of
    ``alpha``, ``span``, ``halflife`` and ``tau``.  ``state``: ``y[-1]`` as a ``float64`` device
    tensor of ``channels`` values (default zeros; pass ``x[0]`` for the ``y[-1] = x[0]``
    convention).  ``return_state``: return ``(y, state)`` with ``y[last frame]`` in fp64 -- the
    next chunk's ``state``; chunked calls reproduce the one-shot output to the accuracy bar of
    include/mavg.h, not bitwise."""
    torch = _torch()
    ema_alpha(alpha, span, halflife, tau)
    _check_device_x(x)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    _ema_state_ptr(state, C, "state")
    like = x.new_empty(0, dtype=torch.float32)  # _with_out's model: x's device, float32
    sout = []

    def into(out):
        if return_state:
            sout.append(_on_stream(stream, lambda: torch.zeros(C, dtype=torch.float64, device=x.device)))
        exponential_moving_average_into(x, out, alpha, span=span, halflife=halflife, tau=tau, channels=C, state=state,
                                        state_out=sout[0] if sout else None, stream=stream, workspace=workspace,
                                        library=library)

    out = _with_out(like, stream, into, (x, state), tuple(x.shape))
    if return_state and x.numel() == 0 and state is not None:
        sout[0].copy_(state)
    return (out, sout[0]) if return_state else out


def biquad_coef(coef):
    """``(b0, b1, b2, a1, a2)`` as five floats from 5 numbers, or from a scipy-style row of 6
    ``(b0, b1, b2, a0, a1, a2)``, which is divided by ``a0`` (``a0 == 0`` is rejected)."""
    import math
    try:
        c = [float(v) for v in (coef.tolist() if hasattr(coef, "tolist") else coef)]
    except TypeError:
        raise ValueError("coef must be 5 numbers (b0 b1 b2 a1 a2) or a row of 6 (b0 b1 b2 a0 a1 a2)") from None
    if len(c) == 6:
        a0 = c[3]
        if a0 == 0.0 or not math.isfinite(a0):
            raise ValueError(f"a0 must be finite and non-zero, got {a0}")
        c = [c[0] / a0, c[1] / a0, c[2] / a0, c[4] / a0, c[5] / a0]
    if len(c) != 5:
        raise ValueError(f"coef must be 5 numbers (b0 b1 b2 a1 a2) or a row of 6 (b0 b1 b2 a0 a1 a2), got {len(c)}")
    if not all(math.isfinite(v) for v in c):
        raise ValueError(f"the coefficients must be finite, got {c}")
    if not (abs(c[4]) < 1.0 and abs(c[3]) < 1.0 + c[4]):
        raise ValueError(f"the poles must lie strictly inside the unit circle (|a2| < 1 and |a1| < 1 + a2), got a1={c[3]} a2={c[4]}")
    return tuple(c)


def _coef5(coef):
    import ctypes
    return (ctypes.c_double * 5)(*biquad_coef(coef))


def biquad_halo_frames(coef, library: Optional[str] = None) -> int:
    """``H``: a frame count past which the impulse response sums to at most ``2**-30`` of its
    whole (include/mavg.h "Halo") -- how far back ``biquad_tile`` reads to rebuild a tile's state."""
    import ctypes
    out = ctypes.c_longlong(0)
    _lib.check(_lib.load(library).mavg_biquad_halo_frames(_coef5(coef), ctypes.byref(out)), "mavg_biquad_halo_frames")
    return out.value


def biquad_workspace_bytes(n: int, coef, channels: int = 1, dtype: int = F32, library: Optional[str] = None) -> int:
    """Device workspace ``biquad_into`` needs: 0 for ``biquad_tile``, two fp64 values per
    1024-frame tile (``biquad_chain``) or per strip (``biquad_strip``) and channel."""
    import ctypes
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_biquad_workspace_bytes(n, channels, _coef5(coef), dtype, ctypes.byref(out)),
               "mavg_biquad_workspace_bytes")
    return out.value


def biquad_plan(n: int, coef, channels: int = 1, dtype: int = F32, state: bool = False, return_state: bool = False,
                library: Optional[str] = None, aligned: bool = True) -> str:
    """What mavg_biquad_run would do (nothing is launched): ``biquad_tile<...> halo_frames=H ...
    tile_frames=N ...``, ``biquad_chain<...> ... records=R carry_chunk=K launches=3`` or
    ``biquad_strip ... L=...``.  ``aligned=False``: for views off 16-B alignment (``F=1``)."""
    import ctypes
    buf = ctypes.create_string_buffer(512)
    flags = (1 if state else 0) | (2 if return_state else 0) | (0 if aligned else 4)
    _lib.check(_lib.load(library).mavg_biquad_plan(n, channels, _coef5(coef), dtype, flags, buf, len(buf)),
               "mavg_biquad_plan")
    return buf.value.decode()


def _biquad_state_shape(state, C: int, what: str) -> None:
    torch = _torch()
    if state is None:
        return
    if state.dtype != torch.float64:
        raise ValueError(f"{what} must be float64 (the state is kept in fp64), got {state.dtype}")
    if state.numel() != 2 * C:
        raise ValueError(f"{what} must hold channels x 2 = {2 * C} values, got {state.numel()}")


def _biquad_state_ptr(state, C: int, what: str):
    """The state's device pointer (None without one); _biquad_state_shape has seen it."""
    if state is None:
        return None
    if not state.is_cuda or not state.is_contiguous():
        raise ValueError(f"{what} must be a contiguous device tensor")
    return state.data_ptr()


def biquad_into(x, out, coef, channels: int = 1, state=None, state_out=None, stream=None, workspace=None,
                library: Optional[str] = None) -> None:
    """Enqueue ``out = biquad(x)`` on ``stream`` (default: current).

    ``out``: a contiguous ``float32`` device tensor of ``x``'s size that does not overlap ``x``.
    ``state`` / ``state_out``: ``float64`` device tensors of ``[channels, 2]`` values -- the
    transposed direct form II's ``s1, s2`` before the first frame, and where those after the last
    go; not the same tensor.  ``workspace``: as in ``exponential_moving_average_into``;
    ``biquad_chain`` and ``biquad_strip`` need one (``biquad_workspace_bytes``)."""
    torch = _torch()
    c5 = _coef5(coef)
    frames, C = _decim_shape(x, channels)
    dt = _dtype_code(x)
    if out.dtype != torch.float32:
        raise ValueError(f"out must be float32 (the biquad is fp32 for every input dtype), got {out.dtype}")
    if out.numel() != x.numel():
        raise ValueError(f"out must hold x's {x.numel()} samples, got {out.numel()}")
    _biquad_state_shape(state, C, "state")
    _biquad_state_shape(state_out, C, "state_out")
    _check_device_pair(x, out)
    sin = _biquad_state_ptr(state, C, "state")
    sout = _biquad_state_ptr(state_out, C, "state_out")
    if sin is not None and sin == sout:
        raise ValueError("state and state_out must not be the same tensor")
    lib = _lib.load(library)
    ws_n = biquad_workspace_bytes(x.numel(), tuple(c5), C, dt, library)
    ws, ws_n = _loop_workspace(ws_n, workspace, stream, x.device, "biquad_workspace_bytes")
    st = lib.mavg_biquad_run(x.data_ptr(), out.data_ptr(), x.numel(), C, c5, dt, sin, sout,
                             ws.data_ptr() if ws is not None else None, ws_n, _stream_handle(stream, x.device))
    _lib.check(st, "mavg_biquad_run")


def biquad(x, coef, channels: int = 1, state=None, return_state: bool = False, stream=None, workspace=None,
           library: Optional[str] = None):
    """``y[f] = b0 x[f] + b1 x[f-1] + b2 x[f-2] - a1 y[f-1] - a2 y[f-2]`` per channel of ``x`` (fp32
    or int16), as ``float32`` in ``x``'s shape.  ``coef``: ``(b0, b1, b2, a1, a2)`` or a scipy-style
    row ``(b0, b1, b2, a0, a1, a2)``; the poles must lie strictly inside the unit circle.
    ``state``: ``scipy.signal.lfilter``'s ``zi`` per channel, a ``float64`` device tensor of
    ``[channels, 2]`` values (default zeros).  ``return_state``: return ``(y, state)`` with the
    state after the last frame -- the next chunk's ``state``; chunked calls reproduce the one-shot
    output to the accuracy bar of include/mavg.h, not bitwise."""
    torch = _torch()
    biquad_coef(coef)
    _check_device_x(x)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    _biquad_state_shape(state, C, "state")
    _biquad_state_ptr(state, C, "state")
    like = x.new_empty(0, dtype=torch.float32)  # _with_out's model: x's device, float32
    sout = []

    def into(out):
        if return_state:
            sout.append(_on_stream(stream, lambda: torch.zeros((C, 2), dtype=torch.float64, device=x.device)))
        biquad_into(x, out, coef, channels=C, state=state, state_out=sout[0] if sout else None, stream=stream,
                    workspace=workspace, library=library)

    out = _with_out(like, stream, into, (x, state), tuple(x.shape))
    if return_state and x.numel() == 0 and state is not None:
        sout[0].copy_(state.reshape(C, 2))
    return (out, sout[0]) if return_state else out


def sos_filter(x, sos, channels: int = 1, state=None, return_state: bool = False, stream=None,
               library: Optional[str] = None):
    """A cascade of second-order sections (``scipy.signal.sosfilt``): ``sos`` is ``[S, 6]`` rows
    ``(b0, b1, b2, a0, a1, a2)``, run one ``mavg_biquad_run`` each through two ping-pong fp32
    buffers -- the first section reads ``x`` in its dtype, the later ones fp32, the last lands in the
    result.  THE INTERMEDIATE BETWEEN SECTIONS IS fp32 (one rounding per section, about ``2**-24``
    of the intermediate's size); a cascade that needs an fp64 intermediate is not this function.
    ``state``: a ``float64`` device tensor ``[S, channels, 2]`` (``sosfilt``'s ``zi`` with the
    channel axis second); ``return_state``: return ``(y, state)`` of that shape.  ``sosfilt`` is
    the cascade in one library call, with an fp64 intermediate wherever its fused kernel fits."""
    torch = _torch()
    rows = sos.tolist() if hasattr(sos, "tolist") else [list(r) for r in sos]
    if not rows or any(not hasattr(r, "__len__") or len(r) != 6 for r in rows):
        raise ValueError("sos must be a non-empty [S, 6] array of (b0, b1, b2, a0, a1, a2) rows")
    coefs = [biquad_coef(r) for r in rows]
    S = len(coefs)
    _check_device_x(x)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    if state is not None:
        if state.dtype != torch.float64 or state.numel() != S * C * 2 or not state.is_cuda or not state.is_contiguous():
            raise ValueError(f"state must be a contiguous float64 device tensor of [sections, channels, 2] = "
                             f"[{S}, {C}, 2] values")
        state = state.reshape(S, C, 2)
    like = x.new_empty(0, dtype=torch.float32)  # _with_out's model: x's device, float32
    sout = []

    def into(out):
        if return_state:
            sout.append(_on_stream(stream, lambda: torch.zeros((S, C, 2), dtype=torch.float64, device=x.device)))
        other = _on_stream(stream, lambda: torch.empty_like(out)) if S > 1 else None
        cur = x
        for j, c in enumerate(coefs):
            dst = out if (S - 1 - j) % 2 == 0 else other      # the last section lands in the result
            biquad_into(cur, dst, c, channels=C, state=state[j] if state is not None else None,
                        state_out=sout[0][j] if sout else None, stream=stream, library=library)
            cur = dst
        if other is not None and stream is not None:
            other.record_stream(stream)

    out = _with_out(like, stream, into, (x, state), tuple(x.shape))
    if return_state and x.numel() == 0 and state is not None:
        sout[0].copy_(state)
    return (out, sout[0]) if return_state else out


def _sos_rows(sos):
    """``sos`` -- a scipy ``[S, 6]`` array of ``(b0, b1, b2, a0, a1, a2)`` rows -- as ``(S, the S x 5
    host doubles mavg_sos_run reads)``, every row normalised and checked by ``biquad_coef``."""
    import ctypes
    rows = sos.tolist() if hasattr(sos, "tolist") else [list(r) for r in sos]
    if not rows or any(not hasattr(r, "__len__") or len(r) != 6 for r in rows):
        raise ValueError("sos must be a non-empty [S, 6] array of (b0, b1, b2, a0, a1, a2) rows")
    flat = [v for r in rows for v in biquad_coef(r)]
    return len(rows), (ctypes.c_double * len(flat))(*flat)


def _sos_flags(intermediate: str) -> int:
    if intermediate not in ("auto", "fp64"):
        raise ValueError(f"intermediate must be 'auto' or 'fp64', got {intermediate!r}")
    return _lib.SOS_FP64_ONLY if intermediate == "fp64" else 0


def sos_halo_frames(sos, library: Optional[str] = None) -> int:
    """The sum of the sections' ``biquad_halo_frames``: how far back ``sos_tile`` stages."""
    import ctypes
    S, c = _sos_rows(sos)
    out = ctypes.c_longlong(0)
    _lib.check(_lib.load(library).mavg_sos_halo_frames(c, S, ctypes.byref(out)), "mavg_sos_halo_frames")
    return out.value


def sos_workspace_bytes(n: int, sos, channels: int = 1, dtype: int = F32, intermediate: str = "auto",
                        library: Optional[str] = None) -> int:
    """Device workspace ``sosfilt_into`` needs: the sections' tables for ``sos_tile``, one or two
    fp32 buffers of the signal's size and the sections' own for ``sos_loop``."""
    import ctypes
    S, c = _sos_rows(sos)
    out = ctypes.c_size_t(0)
    _lib.check(_lib.load(library).mavg_sos_workspace_bytes(n, channels, c, S, dtype, _sos_flags(intermediate),
                                                           ctypes.byref(out)), "mavg_sos_workspace_bytes")
    return out.value


def sos_plan(n: int, sos, channels: int = 1, dtype: int = F32, state: bool = False, return_state: bool = False,
             intermediate: str = "auto", library: Optional[str] = None, aligned: bool = True) -> str:
    """What mavg_sos_run would do (nothing is launched): ``sos_none biquad_...`` for one section,
    ``sos_tile<...> sections=S intermediate=f64 ... tile_frames=N ... launches=1+S`` or ``sos_loop
    ... intermediate=f32 ...``.  ``aligned=False``: for views off 16-B alignment (``F=1``)."""
    import ctypes
    S, c = _sos_rows(sos)
    buf = ctypes.create_string_buffer(512)
    flags = (_sos_flags(intermediate) | (_lib.SOS_PLAN_STATE_IN if state else 0)
             | (_lib.SOS_PLAN_STATE_OUT if return_state else 0) | (0 if aligned else _lib.SOS_PLAN_UNALIGNED))
    _lib.check(_lib.load(library).mavg_sos_plan(n, channels, c, S, dtype, flags, buf, len(buf)), "mavg_sos_plan")
    return buf.value.decode()


def _sos_state_ptr(state, S: int, C: int, what: str):
    torch = _torch()
    if state is None:
        return None
    if state.dtype != torch.float64 or state.numel() != S * C * 2 or not state.is_cuda or not state.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float64 device tensor of [sections, channels, 2] = "
                         f"[{S}, {C}, 2] values")
    return state.data_ptr()


def sosfilt_into(x, out, sos, channels: int = 1, state=None, state_out=None, intermediate: str = "auto", stream=None,
                 workspace=None, library: Optional[str] = None) -> None:
    """Enqueue ``out = sosfilt(sos, x)`` on ``stream`` (default: current): one ``mavg_sos_run``.

    ``out``: a contiguous ``float32`` device tensor of ``x``'s size that does not overlap ``x``.
    ``state`` / ``state_out``: ``float64`` device tensors of ``[sections, channels, 2]`` values, not
    the same tensor.  ``intermediate="fp64"`` raises (``MAVG_ERR_UNSUPPORTED``) where the library
    would run the per-section loop with its fp32 intermediate.  ``workspace``: as in
    ``biquad_into`` (``sos_workspace_bytes``)."""
    torch = _torch()
    S, c = _sos_rows(sos)
    flags = _sos_flags(intermediate)
    frames, C = _decim_shape(x, channels)
    dt = _dtype_code(x)
    if out.dtype != torch.float32:
        raise ValueError(f"out must be float32 (the cascade is fp32 for every input dtype), got {out.dtype}")
    if out.numel() != x.numel():
        raise ValueError(f"out must hold x's {x.numel()} samples, got {out.numel()}")
    _check_device_pair(x, out)
    sin = _sos_state_ptr(state, S, C, "state")
    sout = _sos_state_ptr(state_out, S, C, "state_out")
    if sin is not None and sin == sout:
        raise ValueError("state and state_out must not be the same tensor")
    import ctypes
    lib = _lib.load(library)
    need = ctypes.c_size_t(0)
    _lib.check(lib.mavg_sos_workspace_bytes(x.numel(), C, c, S, dt, flags, ctypes.byref(need)), "mavg_sos_workspace_bytes")
    ws, ws_n = _loop_workspace(need.value, workspace, stream, x.device, "sos_workspace_bytes")
    st = lib.mavg_sos_run(x.data_ptr(), out.data_ptr(), x.numel(), C, c, S, dt, flags, sin, sout,
                          ws.data_ptr() if ws is not None else None, ws_n, _stream_handle(stream, x.device))
    _lib.check(st, "mavg_sos_run")


def sosfilt(x, sos, channels: int = 1, state=None, return_state: bool = False, intermediate: str = "auto", stream=None,
            workspace=None, library: Optional[str] = None):
    """``scipy.signal.sosfilt`` per channel of ``x`` (fp32 or int16), as ``float32`` in ``x``'s
    shape, in one library call: ``sos`` is ``[S, 6]`` rows ``(b0, b1, b2, a0, a1, a2)``.  Where the
    fused kernel fits (one or two channels, up to 16 sections, a total halo of at most 16 KiB of
    fp64: ``sos_plan`` says ``sos_tile``) the intermediate between sections is fp64 and only the
    result is rounded to fp32; elsewhere the library loops over the sections with an fp32
    intermediate, as ``sos_filter`` does, and ``intermediate="fp64"`` raises instead.  ``state``: a
    ``float64`` device tensor ``[S, channels, 2]`` (``sosfilt``'s ``zi`` with the channel axis
    second); ``return_state``: return ``(y, state)`` of that shape."""
    torch = _torch()
    S, _ = _sos_rows(sos)
    _sos_flags(intermediate)
    _check_device_x(x)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    _sos_state_ptr(state, S, C, "state")
    like = x.new_empty(0, dtype=torch.float32)  # _with_out's model: x's device, float32
    sout = []

    def into(out):
        if return_state:
            sout.append(_on_stream(stream, lambda: torch.zeros((S, C, 2), dtype=torch.float64, device=x.device)))
        sosfilt_into(x, out, sos, channels=C, state=state, state_out=sout[0] if sout else None,
                     intermediate=intermediate, stream=stream, workspace=workspace, library=library)

    out = _with_out(like, stream, into, (x, state), tuple(x.shape))
    if return_state and x.numel() == 0 and state is not None:
        sout[0].copy_(state.reshape(S, C, 2))
    return (out, sout[0]) if return_state else out


def fir_taps(taps, device):
    """The taps as mavg_fir_run reads them: a contiguous ``float64`` tensor on ``device``.  A list,
    numpy array or host tensor is checked to be 1-D, non-empty and finite and copied there (any
    dtype: the values are converted to fp64); a ``float64`` device tensor passes through unread --
    the library never reads taps on the host, so non-finite device taps give non-finite outputs."""
    torch = _torch()
    if torch.is_tensor(taps) and taps.is_cuda:
        if taps.dtype != torch.float64:
            raise ValueError(f"device taps must be float64 (the kernels read fp64 taps), got {taps.dtype}")
        if taps.dim() != 1 or taps.numel() < 1:
            raise ValueError(f"taps must be 1-D and non-empty, got shape {tuple(taps.shape)}")
        if taps.device != torch.device(device):
            raise ValueError(f"taps are on {taps.device}, the signal on {torch.device(device)}")
        return taps.contiguous()
    if torch.is_tensor(taps):
        t = taps.detach().to(torch.float64)
    else:
        import numpy as np
        t = torch.from_numpy(np.array(taps, dtype=np.float64))     # a copy: the caller's array may be read-only
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"taps must be 1-D and non-empty, got shape {tuple(t.shape)}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError("taps must be finite")
    return t.contiguous().to(device)


def fir_plan(n: int, ntaps: int, channels: int = 1, dtype: int = F32, history: bool = False, aligned: bool = True,
             library: Optional[str] = None) -> str:
    """What mavg_fir_run would do (nothing is launched): ``fir_tile<...> taps=T halo_frames=T-1 ...
    tile_frames=N ...`` or ``fir_strip ... L=...``.  ``aligned=False``: for views off 16-B alignment
    (``F=1``)."""
    import ctypes
    buf = ctypes.create_string_buffer(512)
    flags = (1 if history else 0) | (0 if aligned else 4)
    _lib.check(_lib.load(library).mavg_fir_plan(n, channels, ntaps, dtype, flags, buf, len(buf)), "mavg_fir_plan")
    return buf.value.decode()


def fir_filter_into(x, out, taps, channels: int = 1, history=None, stream=None, library: Optional[str] = None) -> None:
    """Enqueue ``out = fir_filter(x)`` on ``stream`` (default: current), one launch, no workspace.

    ``out``: a contiguous ``float32`` device tensor of ``x``'s size that does not overlap ``x``.
    ``taps``: as ``fir_taps`` takes them (pass its result to keep host taps from being copied on
    every call).  ``history``: the ``(ntaps-1) * channels`` samples in front of ``x``."""
    torch = _torch()
    frames, C = _decim_shape(x, channels)
    dt = _dtype_code(x)
    if out.dtype != torch.float32:
        raise ValueError(f"out must be float32 (the filter is fp32 for every input dtype), got {out.dtype}")
    if out.numel() != x.numel():
        raise ValueError(f"out must hold x's {x.numel()} samples, got {out.numel()}")
    _check_device_pair(x, out)
    # (host taps are copied on the launch stream, which then owns their block)
    h = _on_stream(stream, lambda: fir_taps(taps, x.device))
    ntaps = h.numel()
    hist_ptr = _history_ptr(history, x, (ntaps - 1) * C, "(ntaps-1)*channels")
    st = _lib.load(library).mavg_fir_run(x.data_ptr(), out.data_ptr(), x.numel(), C, h.data_ptr(), ntaps, dt, hist_ptr,
                                         _stream_handle(stream, x.device))
    _lib.check(st, "mavg_fir_run")


def fir_filter(x, taps, channels: int = 1, history=None, stream=None, library: Optional[str] = None):
    """``y[f] = sum_j taps[j] x[f-j]`` per channel of ``x`` (fp32 or int16), as ``float32`` in
    ``x``'s shape; ``taps[0]`` multiplies the newest frame.  Every output is the fp32 rounding of one
    fp64 fma chain, oldest frame first, so every path, alignment and chunking with a ``history``
    (the ``(ntaps-1) * channels`` samples in front of ``x``) gives the same bits."""
    torch = _torch()
    _check_device_x(x)
    _decim_shape(x, channels)
    _dtype_code(x)
    C = channels if x.dim() == 1 else x.shape[1]
    h = fir_taps(taps, x.device)
    like = x.new_empty(0, dtype=torch.float32)  # _with_out's model: x's device, float32

    def into(out):
        fir_filter_into(x, out, h, channels=C, history=history, stream=stream, library=library)

    return _with_out(like, stream, into, (x, history, h), tuple(x.shape))


def fill_synthetic(n: int, dtype=None, seed: int = 0x5EED, offset: int = 0, dist: int = 0,
                   device="cuda", stream=None, out=None):
    """Counter-based synthetic signal generated on the device:
    element i is splitmix64(seed + offset + i) >> 48 as int16 (dist 0), or a
    uniform [0,1) float (dist 1)."""
    torch = _torch()
    dtype = torch.float32 if dtype is None else dtype
    if out is None:
        out = torch.empty(n, dtype=dtype, device=device)
    st = _lib.load().mavg_fill_synthetic(out.data_ptr(), out.numel(), _dtype_code(out), seed, offset,
                                         dist, _stream_handle(stream, out.device))
    _lib.check(st, "mavg_fill_synthetic")
    return out


def stream_copy(src, dst, stream=None) -> None:
    """HBM calibration: dst = src with the library's flat non-temporal copy
    kernel (not part of the filter; bench.py's same-box streaming ceiling)."""
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != nbytes:
        raise ValueError("src and dst must have the same size in bytes")
    st = _lib.load().mavg_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, _stream_handle(stream, src.device))
    _lib.check(st, "mavg_stream_copy")
