"""Worker for tests/test_gpu_optim.py: the multi-tensor optimizer kernels in a fresh process.

    P2_MT_FASTDIV=0 python tests/optim_fastdiv_worker.py OUT.pt

``csrc/optim.hip`` reads ``P2_MT_FASTDIV`` once per process, so the arm that
computes the channels-last index by integer division (``adam_mt_kernel<false>``
/ ``sgd_mt_kernel<false>``) needs a process of its own.  The worker runs
``optim_cases.run_fastdiv_cases`` -- the whole multi-tensor layout under every
hyperparameter set -- and saves ``{case: {p, m, v | buf, shadow}}`` (CPU
tensors) to ``OUT.pt``; the test holds them against the default arm's bits.
"""

from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import optim_cases as oc  # noqa: E402


def main(out: str) -> None:
    from p2pfl_amd import ops

    ops.ext()
    res = oc.run_fastdiv_cases(ops, torch.device("cuda", 0))
    torch.cuda.synchronize()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1])
