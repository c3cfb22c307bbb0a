"""The compacting end of the decimated tile scan (csrc/mavg_decim.hpp decim_scan_kernel), its
index math restated in numpy on the CPU with the kernel's own 32-bit steps:

- decim_tile_range: once per workgroup, the tile [t0, t0 + tl) -> the first kept output index
  m_lo (the one 64-bit divide), the tile-local index l0 of that frame (TF when it lies past the
  tile) and the number of kept frames cnt (a 32-bit divide);
- decim_first + the walk over a lane unit's F frames: the first kept frame at or after the
  unit's first frame and its slot, then `first += hop, slot += 1` per kept frame.

Checked exhaustively over small tiles: the kept frames are exactly range(phase, n, hop), the
slots are a bijection onto [0, cnt), cnt never exceeds the compaction buffer's TF/2 + 1 frames
(hop >= 2), and consecutive tiles' output ranges abut.  The GPU kernel itself is checked against
the oracle in tests/test_gpu_decim.py."""
import numpy as np
import pytest

U32 = np.uint32


def tile_range(t0, tl, TF, hop, phase):
    """decim_tile_range: (m_lo, l0, cnt); t0 and m_lo are 64-bit, the rest uint32."""
    m_lo = (t0 - phase + hop - 1) // hop if t0 > phase else 0
    d = phase + m_lo * hop - t0
    assert d >= 0
    l0 = U32(d) if d < TF else U32(TF)
    cnt = (U32(tl) - l0 + U32(hop) - U32(1)) // U32(hop) if l0 < U32(tl) else U32(0)
    return m_lo, l0, cnt


def lane_first(i0, l0, hop):
    """decim_first: (first, slot), uint32 steps."""
    i0, l0, hop = U32(i0), U32(l0), U32(hop)
    if i0 <= l0:
        return l0, U32(0)
    slot = (i0 - l0 + hop - U32(1)) // hop
    return l0 + slot * hop, slot


def tile_kept(t0, tl, TF, F, hop, phase):
    """{slot: frame} of one tile, walked unit by unit as the kernel's lanes do."""
    m_lo, l0, cnt = tile_range(t0, tl, TF, hop, phase)
    kept = {}
    if cnt == 0:  # the kernel returns before it loads
        return m_lo, 0, kept
    for i0 in range(0, TF, F):  # one lane unit: F consecutive frames
        first, slot = lane_first(i0, l0, hop)
        for fr in range(F):
            i = U32(i0 + fr)
            if i == first and i < U32(tl):
                assert slot < cnt and int(slot) not in kept
                kept[int(slot)] = t0 + int(i)
                first = first + U32(hop)
                slot = slot + U32(1)
    return m_lo, int(cnt), kept


def check_signal(n, TF, F, hop, phase, tiles=None):
    ntiles = (n + TF - 1) // TF
    next_m = None
    for t in (range(ntiles) if tiles is None else tiles):
        t0 = t * TF
        tl = min(TF, n - t0)
        m_lo, cnt, kept = tile_kept(t0, tl, TF, F, hop, phase)
        assert cnt <= TF // 2 + 1, (TF, hop, phase, t, cnt)
        # the frames of range(phase, n, hop) inside the tile, and how many lie before it
        want = [f for f in range(t0, t0 + tl) if f >= phase and (f - phase) % hop == 0]
        assert m_lo == len(range(phase, t0, hop)), (TF, hop, phase, t)
        if next_m is not None:
            assert m_lo == next_m, (TF, hop, phase, t)  # consecutive tiles' ranges abut
        next_m = m_lo + cnt
        assert sorted(kept) == list(range(cnt)), (TF, F, hop, phase, t)  # a bijection onto [0, cnt)
        assert [kept[s] for s in range(cnt)] == want, (TF, F, hop, phase, t)
    if tiles is None or tiles[-1] == ntiles - 1:
        assert next_m == len(range(phase, n, hop))


@pytest.mark.parametrize("F", (1, 2, 4, 8))
@pytest.mark.parametrize("TF", (16, 64))
def test_kept_frames_and_slots_exhaustively(TF, F):
    """Every hop in 2 .. 2*TF + 1 and every phase, over three tiles and a partial fourth."""
    for hop in range(2, 2 * TF + 2):
        for phase in range(hop):
            check_signal(3 * TF + 5, TF, F, hop, phase)


@pytest.mark.parametrize("TF,F", ((16, 4), (64, 8), (64, 1)))
def test_tiles_far_into_the_signal(TF, F):
    """Several t0, up to past 2^32 and 2^40 frames (t0 and m_lo are the 64-bit values), with a
    partial last tile."""
    for base in (0, 7, 1 << 20, (1 << 32) // TF + 3, (1 << 40) // TF + 11):
        n = (base + 2) * TF + TF // 2 + 1  # tiles base, base + 1 whole, base + 2 partial
        for hop in (2, 3, F - 1 if F > 3 else 5, F + 1, TF - 1, TF, TF + 1, 2 * TF + 1):
            for phase in sorted({0, hop // 2, hop - 1}):
                check_signal(n, TF, F, hop, phase, tiles=(base, base + 1, base + 2))


def test_partial_last_tile_lengths():
    TF, F = 16, 4
    for n in range(1, 3 * TF + 1):
        for hop in (2, 3, 5, 16, 17, 33):
            for phase in range(hop):
                check_signal(n, TF, F, hop, phase)


def test_huge_hop_keeps_32_bit_steps_in_range():
    """hop up to 2^31 - 1: l0 + slot * hop and first + hop stay below 2^32."""
    TF, F = 64, 8
    hop = (1 << 31) - 1
    with np.errstate(over="raise"):
        for phase in (0, 5, TF - 1, TF, hop - 1):
            check_signal(3 * TF + 5, TF, F, hop, phase)
            base = hop // TF
            check_signal((base + 2) * TF + 9, TF, F, hop, phase, tiles=(base - 1, base, base + 1))
