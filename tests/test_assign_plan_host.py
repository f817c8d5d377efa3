"""CPU checks of the labels pass's host plan (csrc/gdd_kmeans.hip, assign_plan): which kernel form a
shape takes, with how many waves, which row fetch, which centre chunks and whether the keys are
prefilled, under each GDD_FORCE token. Every form returns the same labels, so only the name tells a
shape that slipped onto another one. No device calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gdd.h GDD_ASSIGN_*
ROWS, X_UNALIGNED, C_UNALIGNED, BF16, TOP2, PADDED = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def lib():
    from gdd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "graph-distillation-for-recommendation_amd",
                                                   "csrc")], check=True)
    return _lib.load()


# (n, dim, k, flags, GDD_FORCE, path): transcribed from the dispatcher as it stood before the plan existed
PATHS = [
    (16384, 40, 454, 0, "", "small/w16/vec"),  # the last small n
    (100, 231, 5, 0, "", "small/w4/scalar"),
    (100, 240, 5, 0, "", "small/w4/vec"),  # the small form's widest rows ...
    (100, 241, 5, 0, "", "tiles/w1/scalar/32x1/prefill"),  # ... at 241 its 4-wave LDS passes 160 KiB
    (3000, 40, 300, 0, "", "small/w16/vec"),
    (3000, 40, 256, 0, "", "small/w8/vec"),
    (3000, 40, 128, 0, "", "small/w4/vec"),
    (3000, 128, 454, 0, "", "small/w8/vec"),  # 16 waves of 128-wide rows do not fit
    # 12 waves, one chunk, plain stores, and still a prefill: the persistent form would need two chunks
    (16385, 40, 454, 0, "", "waves/w12/contig/480x1/prefill"),
    (2449029, 47, 196, 0, "", "waves/w12/contig/224x1"),  # products
    (16385, 47, 196, 0, "", "waves/w12/contig/224x1"),
    (16385, 7, 70, 0, "", "waves/w12/contig/96x1"),
    (16385, 33, 769, 0, "", "waves/w8/contig/800x1/prefill"),
    (153431, 41, 769, 0, "", "waves/w4/contig/224x4/prefill"),  # Reddit: the persistent form's chunk width
    (16385, 48, 2000, 0, "", "waves/w4/contig/256x8/prefill"),
    (16385, 64, 100, 0, "", "persist/128x1"),
    (16385, 64, 200, 0, "", "persist/128x2/prefill"),
    (16385, 64, 1773, 0, "", "persist/160x12/prefill"),
    (16385, 96, 300, 0, "", "persist/64x5/prefill"),
    (16385, 97, 300, 0, "", "tiles/w2/scalar/64x5/prefill"),
    (169343, 128, 454, 0, "", "tiles/w2/vec/32x15/prefill"),  # arxiv
    (16385, 224, 300, 0, "", "tiles/w2/vec/32x10/prefill"),
    (16385, 225, 300, 0, "", "tiles/w1/scalar/128x3/prefill"),
    (153431, 602, 769, 0, "", "tiles/w1/scalar/32x25/prefill"),  # the Lloyd loop's pass takes rows past 512
    (64, 300, 33, 0, "", "tiles/w1/vec/32x2/prefill"),
    # a row list; X not 16-byte aligned; C not 16-byte aligned
    (16384, 40, 454, ROWS, "", "small/w16/vec"),
    (16384, 40, 454, X_UNALIGNED, "", "small/w16/scalar"),
    (16384, 40, 454, C_UNALIGNED, "", "small/w16/scalar"),
    (16385, 40, 454, ROWS, "", "waves/w12/rows/480x1/prefill"),
    (16385, 40, 454, X_UNALIGNED, "", "waves/w12/rows/480x1/prefill"),
    (16385, 40, 454, C_UNALIGNED, "", "waves/w12/contig/480x1/prefill"),
    (16385, 47, 196, ROWS, "", "waves/w12/rows/224x1"),
    (153431, 41, 769, ROWS | X_UNALIGNED, "", "waves/w4/rows/224x4/prefill"),
    (16385, 64, 100, ROWS, "", "persist/128x1"),
    (16385, 64, 200, X_UNALIGNED | C_UNALIGNED, "", "persist/128x2/prefill"),
    (169343, 128, 454, ROWS, "", "tiles/w2/vec/32x15/prefill"),
    (169343, 128, 454, X_UNALIGNED, "", "tiles/w2/scalar/32x15/prefill"),
    (169343, 128, 454, C_UNALIGNED, "", "tiles/w2/scalar/32x15/prefill"),
    # the bounded E-step: every centre in one chunk, any n, never a prefill
    (2449029, 47, 196, TOP2, "", "waves_top2/w12/contig/224x1"),
    (2449029, 47, 196, TOP2 | ROWS, "", "waves_top2/w12/rows/224x1"),
    (2449029, 47, 196, TOP2 | ROWS | PADDED, "", "waves_top2/w12/row4/224x1"),
    (2449029, 47, 196, TOP2 | X_UNALIGNED | PADDED, "", "waves_top2/w12/row4/224x1"),
    (2449029, 47, 196, TOP2 | PADDED, "", "waves_top2/w12/contig/224x1"),
    (1000, 40, 454, TOP2, "", "waves_top2/w12/contig/480x1"),
    (16385, 33, 769, TOP2 | ROWS, "", "waves_top2/w8/rows/800x1"),
    (16385, 41, 769, TOP2, "", "invalid"),  # no wave count holds 769 centres of 41
    (100, 49, 5, TOP2, "", "invalid"),
    # bf16: the r06 kernel's two block forms, the r03 kernel, the tiles
    (50000, 40, 454, BF16, "", "bf16q/w4"),
    (2449029, 47, 196, BF16, "", "bf16q/w4"),
    (40000, 41, 769, BF16, "", "bf16q/w8"),
    (40000, 41, 769, BF16, "bf16_w4", "bf16q/w4"),
    (40000, 41, 769, BF16, "bf16_v1", "bf16p/per6"),
    (9000, 45, 100, BF16, "", "bf16q/w4"),
    (9000, 45, 100, BF16, "bf16_w8", "bf16q/w8"),
    (9000, 45, 100, BF16, "bf16_v1", "bf16p/per6"),
    (9000, 40, 100, BF16, "bf16_w8", "bf16q/w4"),  # 8 waves only at dims 41 .. 47 off multiples of 4
    (20000, 64, 200, BF16, "", "bf16p/per8"),  # dim a multiple of 16
    (20000, 100, 200, BF16, "", "bf16p/per13"),
    (1000, 41, 5, BF16, "", "bf16q/w4"),
    (31, 41, 40, BF16, "", "bf16_tiles/32x2/prefill"),  # the r03 fragments pass 31 keys' workspace
    (3000, 200, 30, BF16, "", "bf16_tiles/32x1/prefill"),
    (40000, 41, 769, BF16 | ROWS, "", "bf16_tiles/256x4/prefill"),
    (40000, 41, 769, BF16 | X_UNALIGNED, "", "bf16_tiles/256x4/prefill"),
    (40000, 41, 769, BF16 | C_UNALIGNED, "", "bf16q/w8"),
    (50000, 40, 3000, BF16, "", "bf16_tiles/416x8/prefill"),  # the centre fragments pass 150 KiB
    # 1100 centres of 47: the 8-wave form's LDS does not fit, the 4-wave form's does (before the plan
    # the call failed, also under bf16_w8)
    (16000, 47, 1100, BF16, "", "bf16q/w4"),
    (16000, 47, 1100, BF16, "bf16_w8", "bf16q/w4"),
    (16000, 47, 1100, BF16, "bf16_v1", "bf16p/per6"),
    (16000, 41, 1280, BF16, "", "bf16q/w4"),
    (16000, 41, 1088, BF16, "", "bf16q/w8"),
    # ... at n = 2048 the queried workspace is smaller than the r03 fragments, which gates both
    # persistent kernels as it did before the plan: the tiles
    (2048, 47, 1100, BF16, "", "bf16_tiles/32x35/prefill"),
    (2048, 47, 1100, BF16, "bf16_w8", "bf16_tiles/32x35/prefill"),
    # the widest dims gdd.h admits: from 497 the four-wave block's LDS (166,544 bytes) is past a CU's,
    # two waves per block hold it (these were "invalid" before; tests/test_gpu_bf16_labels.py runs them)
    (2013, 496, 96, BF16, "", "bf16_tiles/32x3/prefill"),
    (2013, 497, 96, BF16, "", "bf16_tiles/32x3/prefill"),
    (2013, 512, 96, BF16, "", "bf16_tiles/32x3/prefill"),
    (1, 512, 1, BF16, "", "bf16_tiles/32x1/prefill"),
]


@pytest.mark.parametrize("n,dim,k,flags,env,path", PATHS)
def test_path_table(lib, monkeypatch, n, dim, k, flags, env, path):
    if env:
        monkeypatch.setenv("GDD_FORCE", env)
    else:
        monkeypatch.delenv("GDD_FORCE", raising=False)
    assert lib.gdd_kmeans_assign_path(n, dim, k, flags).decode() == path


def test_refused_shapes(lib, monkeypatch):
    monkeypatch.delenv("GDD_FORCE", raising=False)
    for n, dim, k, flags in [(0, 16, 4, 0), (-1, 16, 4, 0), (10, 0, 4, 0), (10, 16, 0, 0), (10, 16, 0, BF16),
                             (10, 513, 4, BF16), (10, 16, 4, BF16 | TOP2), (0, 16, 4, TOP2),
                             (70000, 700, 40, 0)]:
        assert lib.gdd_kmeans_assign_path(n, dim, k, flags) == b"invalid", (n, dim, k, flags)


def _assign_lds(waves, dimp, cch):
    """k_assign_waves' LDS: the centre chunk, 32 point rows per wave, the chunk's norms."""
    return 4 * (cch * (dimp + 1) + 32 * waves * (dimp + 1) + cch)


def test_lloyd_prune_follows_the_plan(lib, monkeypatch):
    """The bounded E-step (lloyd_prune_ok) exists exactly where the wave tiles hold every centre in one
    chunk: the top-2 name is a one-chunk wave-tile name there and "invalid" elsewhere, and the plain
    pass of the same shape at large n has the same waves and chunk."""
    monkeypatch.delenv("GDD_FORCE", raising=False)
    for dim in range(1, 65):
        for k in (1, 33, 196, 454, 769, 1100, 3000):
            kp, dimp = (k + 31) // 32 * 32, (dim + 1) // 2 * 2
            waves = next((w for w in (12, 8, 4) if _assign_lds(w, dimp, kp) <= 150 * 1024), 0) if dim <= 48 else 0
            top2 = lib.gdd_kmeans_assign_path(100000, dim, k, TOP2).decode()
            plain = lib.gdd_kmeans_assign_path(100000, dim, k, 0).decode()
            if waves:
                assert top2 == f"waves_top2/w{waves}/contig/{kp}x1", (dim, k)
                assert plain.startswith(f"waves/w{waves}/contig/{kp}x1"), (dim, k, plain)
            else:
                assert top2 == "invalid", (dim, k)
                assert not plain.startswith("waves/") or not plain.split("/")[3].endswith("x1"), (dim, k, plain)
