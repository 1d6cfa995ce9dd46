"""A handler's life on the GPU returns its device memory: create, a walk, a DES
batch with a span tap under a load profile (every lazily made per-device table
exists by then), free -- over and over, the device's free memory does not go down."""
import pytest

import isim
from isim import native
from isim.yamljson import obj_to_json

pytestmark = pytest.mark.gpu

N = 256
MIB = 1 << 20


def _wide_chain():
    """17 services, each calling the next twice at 50 %, concurrently: a wide tree of 2^17 - 1 positions
    (tests/test_des.py test_des_class), whose walk, item-engine and span tables are each megabytes."""
    out = []
    for i in range(17):
        calls = [{"call": {"service": f"s{i + 1}", "probability": 50}} for _ in range(2)] if i < 16 else []
        out.append({"name": f"s{i}", "isEntrypoint": i == 0, "script": [calls] if calls else []})
    return obj_to_json({"services": out})


def test_handler_lifecycle_returns_device_memory(gpu):
    import torch
    lib = native.load()
    graph = isim.ServiceGraph.from_json(_wide_chain())
    profile = isim.LoadProfile.steps([(2_000_000, 300_000)], 100_000)
    free = lambda: torch.cuda.mem_get_info(gpu)[0]

    def cycle():
        """(free before create - free after the serves, free after the handler is gone)"""
        before = free()
        h = isim.Handler(graph, None, isim.SimParams())
        recs, _ = h.serve(0, N, device=gpu)
        assert len(recs) == N
        d = isim.DesHandler(h, profile=profile)
        assert d.info.items == 1 and d.info.n_positions == (1 << 17) - 1
        recs, _, _, traces, _ = d.serve_spans(0, N, min_latency_ns=0, max_traces=8, cap_spans=1 << 12, device=gpu)
        assert len(recs) == N and traces
        held = before - free()
        lib.isim_handler_free(h._h)
        h._h = None
        return held, free()

    cycle()  # warm-up: the runtime's own first-use allocations (code objects, streams, the pools' first blocks)
    runs = [cycle() for _ in range(3)]   # no torch allocation between the readings
    footprint = min(held for held, _ in runs)
    after = [a for _, a in runs]
    print(f"footprint {[h / MIB for h, _ in runs]} MiB, free after each cycle {after}, "
          f"drift first to third {(after[0] - after[2]) / MIB:.3f} MiB")
    # the graph is chosen so that one table is far above the allocator's granularity
    assert footprint >= 4 * MIB, footprint
    assert after[0] - after[2] <= footprint // 2, (after, footprint)
