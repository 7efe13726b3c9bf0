"""MI355X-native low-level search engine for CBS / ECBS (the one hot path of Sartor02/libMultiRobotPlanning).

Layout:
  csrc/ll_kernel.hip      hand-written gfx950 kernels: A* / focal A*-epsilon over (time, cell) states; job loops, launchers
  csrc/ll_compact.h       the compact (LDS) tier of the CBS / ECBS searches
  csrc/ll_arena_heap.h, ll_arena_search.h, ll_jobs.h, ll_ta.h, ll_sipp.h
                          the arena tier, job staging / runJob / runChain, task assignment, SIPP (included by ll_kernel.hip)
  csrc/ll_launch.h        the one declaration of everything the host launches (kernel parameter records, launchers)
  csrc/mrp_ll_host.cpp    C-ABI (include/mrp_ll.h), the one host translation unit: create / destroy, tiers, statistics
  csrc/host/              its subjects as headers: ll_pack.h + ll_sipp_table.h + ll_unpack.h (HIP-free packer / unpacker),
                          ll_ctx.h (context, job record, collection), ll_maps.h, ll_heur_host.h, ll_stores.h, ll_batch.h,
                          ll_session.h, ll_session_jobs.h, ll_submit.h
  csrc/hl/                host-side C++ conflict-tree drivers (CBS, ECBS) that call the C-ABI (include/mrp_hl.h)
  ll.py / hl.py           ctypes plumbing used by tests and bench.py

The product path never imports ``oracle`` and has no CPU fallback.
"""
import os as _os

# one hardware queue per host worker stream (ROCm default: 4); only effective if set before HIP initialises.  32 covers
# the sixteen resident kernels of eight engines and the runtime's own streams; a smaller inherited value is raised to it
_q = _os.environ.get("GPU_MAX_HW_QUEUES", "")
if not _q.isdigit() or int(_q) < 32:
    _os.environ["GPU_MAX_HW_QUEUES"] = "32"

from . import _build  # noqa: F401,E402

__all__ = ["ll", "hl", "_build"]
