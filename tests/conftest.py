import os
import sys

# xdist runs 4 workers on an 8-core box: cap intra-op threads per worker so
# the model matrix doesn't thrash on oversubscribed OpenMP pools
_omp_preset = os.environ.get('OMP_NUM_THREADS', '')
os.environ.setdefault('OMP_NUM_THREADS', '2')

import pytest
import torch

# a quarter of the usable CPUs per worker, but never more than 4 threads (the
# test models are tiny; on a big shared host cpu_count()//4 gave 4 workers x 64+
# threads fighting over a small CPU share) nor more than OMP_NUM_THREADS allows
_cpus = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 8)
_threads = min(_cpus // 4, 4)
if _omp_preset.isdigit():
    _threads = min(_threads, int(_omp_preset))
torch.set_num_threads(max(1, _threads))

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: test requires a (MI355X) GPU")
    config.addinivalue_line("markers", "base: core model tests")
    config.addinivalue_line("markers", "slow: long-running test")


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip_gpu = pytest.mark.skip(reason="no GPU available")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip_gpu)
