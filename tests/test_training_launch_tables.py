"""CPU checks of what the Adam and keep launches share on the host: the chunk
table (csrc/tensor_chunks.h, through its stand-alone check program built with
the host compiler, no sanitizer here: `make -C csrc chunks-sanitize` is that
build) and the ctypes launch tables (_lib.LaunchTables; only data_ptr and numel
of the CPU tensors are used).
"""
import os
import shutil
import subprocess

import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


def test_chunk_table_against_the_brute_force_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed (csrc/Makefile's HOSTCXX)"
    exe = str(tmp_path / "tensor_chunks_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", os.path.join(CSRC, "tensor_chunks_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.startswith("tensor_chunks_check:") and run.stdout.rstrip().endswith("tables ok")


def _keep_inputs(src, dst):
    return [(s.data_ptr(), d.data_ptr()) for s, d in zip(src, dst)], [s.numel() for s in src]


def test_launch_tables_slice_cache_and_hold():
    src = [torch.zeros(n) for n in (1, 3, 4, 5, 7, 2048, 2049, 11, 13)]
    dst = [torch.zeros_like(s) for s in src]
    tables = _lib.LaunchTables(_lib.KeepTensor, _lib.KEEP_MAX_TENSORS)
    one = tables.launches(*_keep_inputs(src, dst))
    assert [(n, hold) for _, n, hold in one] == [(8, True), (1, False)]   # 9 tensors: 8 + 1, all but the last hold
    rows = [r for tab, n, _ in one for r in tab[:n]]
    assert len(one[0][0]) == 8 and len(one[1][0]) == 1
    assert [(r.src, r.dst, r.numel) for r in rows] == [(s.data_ptr(), d.data_ptr(), s.numel()) for s, d in zip(src, dst)]

    two = tables.launches(*_keep_inputs(src, dst))
    assert all(a[0] is b[0] for a, b in zip(one, two))   # same tensors: the same table objects

    dst[8] = torch.zeros_like(src[8])   # one tensor replaced: only its launch's table is rebuilt
    three = tables.launches(*_keep_inputs(src, dst))
    assert three[0][0] is one[0][0] and three[1][0] is not one[1][0]
    assert (three[1][0][0].src, three[1][0][0].dst, three[1][0][0].numel) == (src[8].data_ptr(), dst[8].data_ptr(), 13)

    tables.clear()
    assert tables.launches(*_keep_inputs(src, dst))[0][0] is not one[0][0]


def test_launch_tables_of_several_groups_number_on_and_hold_to_the_last():
    p = [torch.zeros(4) for _ in range(9)]
    ptrs = [(x.data_ptr(),) * 4 for x in p]
    tables = _lib.LaunchTables(_lib.AdamTensor, _lib.ADAM_MAX_TENSORS)
    a = tables.launches(ptrs, [4] * 9, 0, False)        # a first parameter group: every launch holds the step
    b = tables.launches(ptrs[:2], [4] * 2, len(a), True)   # the last group
    assert [(n, hold) for _, n, hold in a + b] == [(8, True), (1, True), (2, False)]
    assert (b[0][0][1].p, b[0][0][1].v, b[0][0][1].numel) == (p[1].data_ptr(), p[1].data_ptr(), 4)
    again = tables.launches(ptrs, [4] * 9, 0, False) + tables.launches(ptrs[:2], [4] * 2, len(a), True)
    assert all(x[0] is y[0] for x, y in zip(a + b, again))
