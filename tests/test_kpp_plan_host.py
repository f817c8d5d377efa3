"""CPU checks of the k-means++ host plan (csrc/gdd_kmeanspp.hip, kpp_plan): which launch path a shape
takes under each GDD_FORCE token, and the workspace queries that measure the launcher's own layout.
Every path returns the same bits, so only the name tells a shape that slipped onto a slower one.
No device calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from gdd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "graph-distillation-for-recommendation_amd",
                                                   "csrc")], check=True)
    return _lib.load()


# (n, dim, T, k, GDD_FORCE, path): transcribed from the dispatcher as it stood before the plan existed
PATHS = [
    (3000, 128, 8, 454, "", "single_fused/seq"),  # the benchmark's init subset
    (6040, 64, 8, 604, "", "big_pair"),  # ML-1M users
    (17730, 64, 9, 1773, "", "block_table"),  # Ali-Display users
    (2449029, 47, 7, 196, "", "split"),  # products
    (153431, 602, 8, 769, "", "block/blas"),
    (100, 16, 4, 20, "", "single_table_pair"),
    (4096, 64, 8, 16, "", "single_table_pair"),
    (4096, 65, 8, 16, "", "single_fused/seq"),
    (1000, 16, 4, 15, "", "single_fused/seq"),
    (1000, 16, 9, 16, "", "single_table"),
    (1000, 16, 4, 16, "kpp_single_round", "single_table"),
    (1000, 16, 4, 16, "kpp_no_table", "single_fused/seq"),
    (1000, 16, 4, 16, "kpp_no_table,kpp_two_launch", "single_two_launch/seq"),
    (3000, 400, 4, 20, "", "single_fused/blas"),
    (3000, 600, 4, 20, "", "single_two_launch/blas"),
    (4096, 16, 16, 8, "", "single_fused/seq"),
    (4000, 40, 1, 8, "", "block/blas"),
    (4097, 64, 4, 20, "", "block/seq"),
    (4097, 64, 4, 20, "kpp_force_table", "big_pair"),
    (4097, 8, 4, 20, "", "big_pair"),
    (4097, 8, 4, 20, "kpp_force_table,kpp_single_round", "big"),
    (4097, 8, 4, 20, "kpp_force_table,kpp_no_big1", "block_table"),
    (4097, 8, 12, 20, "kpp_force_table", "block/blas"),
    (8193, 8, 4, 20, "kpp_force_table", "big"),
    (9000, 24, 4, 200, "", "big"),
    (9000, 24, 4, 200, "kpp_no_big1", "block_table"),
    (16385, 8, 4, 20, "kpp_force_table", "block_table"),
    (16385, 8, 4, 20, "kpp_force_table,kpp_big1_max=32768", "big"),
    (20000, 24, 4, 2000, "", "block_table"),
    (32769, 8, 4, 2000, "", "block/seq"),
    (40000, 16, 4, 50, "", "block/seq"),
    (530000, 8, 4, 16, "", "split"),
    (530000, 8, 4, 16, "kpp_no_split", "block/seq"),
    (524288, 8, 9, 16, "", "block/seq"),
]


@pytest.mark.parametrize("n,dim,T,k,env,path", PATHS)
def test_path_table(lib, monkeypatch, n, dim, T, k, env, path):
    if env:
        monkeypatch.setenv("GDD_FORCE", env)
    else:
        monkeypatch.delenv("GDD_FORCE", raising=False)
    assert lib.gdd_kmeans_plusplus_path(n, dim, T, k).decode() == path


def test_path_of_one_centre_and_of_refused_shapes(lib, monkeypatch):
    monkeypatch.delenv("GDD_FORCE", raising=False)
    assert lib.gdd_kmeans_plusplus_path(1000, 16, 4, 1) == b"first_only"
    for n, dim, T, k in [(0, 16, 4, 1), (10, 0, 4, 2), (10, 16, 0, 2), (10, 16, 17, 2), (10, 16, 4, 11),
                         (10, 4097, 4, 2), (10, 16, 4, 0)]:
        assert lib.gdd_kmeans_plusplus_path(n, dim, T, k) == b"invalid"


@pytest.mark.parametrize("n", [100, 4096, 4097, 8193, 20000, 32768, 32769])
def test_workspace_grows_with_k_and_stays_under_the_bound(lib, monkeypatch, n):
    monkeypatch.delenv("GDD_FORCE", raising=False)
    for dim in (8, 64, 65):
        for T in (1, 4, 9):
            sizes = [lib.gdd_kmeans_plusplus_ws_bytes_k(n, dim, T, k) for k in sorted({1, 2, 15, 16, 200, n})]
            assert sizes == sorted(sizes), (n, dim, T, sizes)
            at_n = lib.gdd_kmeans_plusplus_ws_bytes_k(n, dim, T, n)
            assert at_n <= lib.gdd_kmeans_plusplus_ws_bytes(n, dim, T), (n, dim, T)
