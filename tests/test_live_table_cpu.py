"""CPU side of the live-range optimizer step: ``build_live_chunks`` turns tap
windows into the chunk table ``(start, run_len, run_pitch, nruns)`` the
``*_live`` kernels index the flat buffers with, unchecked.  The table is
expanded element by element here and compared with a mask filled by brute
force from the definition of a tap window."""
import numpy as np
import pytest

from horizonml_amd.engine.flat import LIVE_CHUNK, build_live_chunks


def _brute_mask(numel, windows):
    live = np.ones(numel, dtype=bool)
    for off, K, Rf, Sf, C, r0, R, s0, S in windows:
        for k in range(K):
            for r in range(Rf):
                for s in range(Sf):
                    if not (r0 <= r < r0 + R and s0 <= s < s0 + S):
                        b = off + ((k * Rf + r) * Sf + s) * C
                        live[b:b + C] = False
    return live


def _expand(numel, chunks, chunk):
    """Times every element is covered; every chunk in bounds and no larger
    than ``chunk``."""
    cover = np.zeros(numel, dtype=np.int64)
    for start, run_len, pitch, nruns in chunks:
        assert run_len >= 1 and nruns >= 1 and start >= 0
        assert run_len * nruns <= chunk
        assert nruns == 1 or pitch >= run_len
        assert start + (nruns - 1) * pitch + run_len <= numel
        for r in range(nruns):
            cover[start + r * pitch:start + r * pitch + run_len] += 1
    return cover


def _check(numel, windows, chunk):
    chunks, n_dead = build_live_chunks(numel, windows, chunk)
    live = _brute_mask(numel, windows)
    cover = _expand(numel, chunks, chunk)
    assert np.array_equal(cover[live], np.ones(int(live.sum()), np.int64)), \
        "a live element is missed or covered twice"
    assert not cover[~live].any(), "a dead element is covered"
    assert n_dead == int((~live).sum())
    return chunks


def _random_layout(rng):
    """Random conv filters with random windows, interleaved with 1-D tensors
    of odd lengths (some missing, so filters also touch)."""
    windows, off = [], 0
    for _ in range(rng.integers(1, 7)):
        if rng.random() < 0.7:
            off += int(rng.choice([1, 3, 7, 10, 129, 515]))
        K, C = int(rng.integers(1, 9)), int(rng.choice([1, 3, 4, 8, 33]))
        Rf, Sf = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        R, S = int(rng.integers(1, Rf + 1)), int(rng.integers(1, Sf + 1))
        r0, s0 = int(rng.integers(0, Rf - R + 1)), int(rng.integers(0, Sf - S + 1))
        windows.append((off, K, Rf, Sf, C, r0, R, s0, S))
        off += K * Rf * Sf * C
    if rng.random() < 0.7:
        off += int(rng.choice([1, 5, 11, 1000]))
    return max(off, 1), windows


@pytest.mark.parametrize("seed", range(40))
def test_random_layouts_cover_live_exactly_once(seed):
    rng = np.random.default_rng(seed)
    numel, windows = _random_layout(rng)
    rng.shuffle(windows)  # the builder sorts by offset itself
    _check(numel, windows, int(rng.choice([1, 5, 64, 256, 4096])))


def test_flagship_layer4_shapes():
    """512-element runs at pitch 4608 (1x1 window of a 3x3x512 filter) and a
    2x2 window of a 3x3x256 filter: the runs are grouped per window row."""
    vec = 515
    w1 = (vec, 64, 3, 3, 256, 1, 2, 1, 2)
    o2 = vec + 64 * 9 * 256 + 64
    w2 = (o2, 32, 3, 3, 512, 1, 1, 1, 1)
    numel = o2 + 32 * 9 * 512 + 10
    chunks = _check(numel, [w1, w2], LIVE_CHUNK)
    grouped = [c for c in chunks if c[3] > 1]
    assert {(c[1], c[2]) for c in grouped} == {(512, 2304), (512, 4608)}
    assert all(c[3] == LIVE_CHUNK // 512 for c in grouped)


def test_full_width_window_is_one_run_per_filter():
    chunks = _check(4 * 3 * 3 * 8, [(0, 4, 3, 3, 8, 1, 1, 0, 3)], 4096)
    assert chunks == [(24, 24, 72, 4)]


def test_no_windows_or_full_windows_have_no_dead_element():
    chunks, n_dead = build_live_chunks(10000, [], 4096)
    assert n_dead == 0 and chunks == [(0, 4096, 0, 1), (4096, 4096, 0, 1),
                                      (8192, 1808, 0, 1)]
    # a fully live filter does not break the span it lies in
    again, n_dead = build_live_chunks(10000, [(7, 8, 3, 3, 8, 0, 3, 0, 3)],
                                      4096)
    assert n_dead == 0 and again == chunks


def test_runs_longer_than_a_chunk_are_cut():
    _check(10 + 2 * 3 * 3 * 700 + 7, [(10, 2, 3, 3, 700, 1, 1, 1, 1)], 256)


@pytest.mark.parametrize("bad", [
    [(0, 2, 3, 3, 4, 1, 3, 0, 1)],                  # window leaves the filter
    [(0, 2, 3, 3, 4, 0, 0, 0, 1)],                  # empty window
    [(90, 2, 3, 3, 4, 1, 1, 1, 1)],                 # filter leaves the buffer
    [(0, 1, 3, 3, 4, 1, 1, 1, 1), (35, 1, 3, 3, 4, 1, 1, 1, 1)],  # overlap
])
def test_bad_geometry_is_refused(bad):
    with pytest.raises(ValueError):
        build_live_chunks(100, bad, 64)
