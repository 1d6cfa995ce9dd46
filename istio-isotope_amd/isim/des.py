"""Per-replica worker-pool DES (BASELINE config 5).

    d = DesHandler(handler, mean_interarrival_ns=6_000_000)
    d = DesHandler(handler, profile=isim.LoadProfile.steps([...], then_mean_ns))   # a time-varying load (§17)
    recs, stats, table = d.serve(trace_begin, n_traces, device=0)
    rows = d.fold(table)      # [n_services][DES_ROW_WORDS]

The simulated counterpart of isotope under load: the client (Fortio's
open-loop mode) issues requests at exponential gaps; each replica of a
service (numReplicas, convert/pkg/graph/svc/service.go:30-31) is a FIFO queue
in front of one worker, or of ``workers`` of them (the
requests a server handles at once).  Statuses/hops/counters are the static walk's;
latencies and per-service durations include queueing.  Runs on the GPU
through libisim (isim_serve_des*); graphs outside the DES class raise
IsimError(EINVAL) with the reason.

Rows are 32-bit by default (times relative to each trace's arrival); a
device batch with a latency of 2^31 ns or more is not accumulated and is
counted in stats[ST_DES_RETRY] — rerun it with ``wide=True``.  ``serve``
does that itself.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native
from .quantiles import DEFAULT_Q
from .sim import REC_DTYPE, Handler


class DesHandler:
    def __init__(self, handler: Handler, mean_interarrival_ns: int = None, profile=None, workers=None):
        """Exactly one of mean_interarrival_ns (a stationary Poisson load) and
        profile (an isim.LoadProfile) is given.  workers (DESIGN.md
        §10.1a): the workers of each replica behind its one queue — an int for
        every service, a {service name: k} dict (the others 1) or an array by
        service index; None leaves the handler's as they are (1 each until
        set).  They are the HANDLER's state (isim_des_workers_set): every
        DesHandler over it serves with them."""
        if (mean_interarrival_ns is None) == (profile is None):
            raise ValueError("DesHandler takes exactly one of mean_interarrival_ns and profile")
        self.handler = handler
        self.profile = profile
        self.params = native.DesParams(int(mean_interarrival_ns), 0, 0) if profile is None else None
        info = native.DesInfo()
        native.check(native.load().isim_des_info_get(handler._h, C.byref(info)))
        self.info = info
        if workers is not None:
            self.workers = workers

    @property
    def workers(self) -> np.ndarray:
        """isim_des_workers_get: u32[n_services], the workers per replica of each service."""
        out = np.zeros(int(self.handler.info.n_services), np.uint32)
        native.check(native.load().isim_des_workers_get(self.handler._h, out.ctypes.data))
        return out

    @workers.setter
    def workers(self, workers) -> None:
        n = int(self.handler.info.n_services)
        if workers is None:
            native.check(native.load().isim_des_workers_set(self.handler._h, None, n))
            return
        if isinstance(workers, dict):
            names = [s["name"] for s in self.handler.graph.canonical()["services"]]
            unknown = sorted(set(workers) - set(names))
            if unknown:
                raise ValueError(f"workers: no service named {unknown[0]!r}")
            workers = [workers.get(name, 1) for name in names]
        elif np.ndim(workers) == 0:
            workers = [workers] * n
        vals = [int(w) for w in workers]
        if any(w < 0 or w > 0xFFFFFFFF for w in vals):
            raise ValueError("workers: a count outside u32")
        w = np.ascontiguousarray(vals, dtype=np.uint32)
        native.check(native.load().isim_des_workers_set(self.handler._h, w.ctypes.data if len(w) else None, len(w)))

    def last_batch(self) -> dict:
        """isim_des_last_batch: the item engine's last batch on this handler
        (passes over the rounds, host synchronisations, executed invocations)."""
        st = native.DesBatchStats()
        native.check(native.load().isim_des_last_batch(self.handler._h, C.byref(st)))
        return {"passes": int(st.passes), "syncs": int(st.syncs), "items": int(st.items)}

    @property
    def table_words(self) -> int:
        return int(self.info.table_rows) * native.DES_ROW_WORDS

    def new_table(self) -> np.ndarray:
        return np.zeros(max(1, self.table_words), np.uint64)

    def workspace_bytes(self, n_traces: int) -> int:
        out = C.c_uint64()
        native.check(native.load().isim_des_workspace_bytes(self.handler._h, n_traces, C.byref(out)))
        return int(out.value)

    def serve(self, trace_begin: int, n_traces: int, device: int = 0, records: bool = True, wide: bool = False):
        """Synchronous: (records or None, stats, DES table)."""
        stats = self.handler.new_stats()
        table = self.new_table()
        recs = np.zeros(n_traces, REC_DTYPE) if records else None
        if self.profile is not None:
            # isim_serve_des_profile starts with 32-bit rows and reruns wide itself: `wide` changes no result
            native.check(native.load().isim_serve_des_profile(
                self.handler._h, device, self.profile.c, trace_begin, n_traces,
                recs.ctypes.data if records and n_traces else None, stats.ctypes.data, table.ctypes.data))
            return recs, stats, table
        p = native.DesParams(self.params.mean_interarrival_ns, native.DES_FLAG_WIDE if wide else 0, 0)
        native.check(native.load().isim_serve_des(
            self.handler._h, device, C.byref(p), trace_begin, n_traces,
            recs.ctypes.data if records and n_traces else None, stats.ctypes.data, table.ctypes.data))
        return recs, stats, table

    def serve_device(self, trace_begin: int, n_traces: int, d_records: int, d_stats: int, d_table: int,
                     d_workspace: int, workspace_bytes: int, stream: int = 0, wide: bool = False) -> None:
        if self.profile is not None:
            native.check(native.load().isim_serve_des_profile_device(
                self.handler._h, self.profile.c, native.DES_FLAG_WIDE if wide else 0, trace_begin, n_traces,
                d_records or None, d_stats, d_table, d_workspace, workspace_bytes, stream or None))
            return
        p = self.params
        if wide:
            p = native.DesParams(p.mean_interarrival_ns, native.DES_FLAG_WIDE, 0)
        native.check(native.load().isim_serve_des_device(
            self.handler._h, C.byref(p), trace_begin, n_traces, d_records or None, d_stats, d_table,
            d_workspace, workspace_bytes, stream or None))

    def _load_args(self, wide: bool):
        """(isim_des_params, isim_load_profile or None) of isim_serve_des_spans*."""
        mean = self.params.mean_interarrival_ns if self.profile is None else 0
        p = native.DesParams(mean, native.DES_FLAG_WIDE if wide else 0, 0)
        return p, (self.profile.c if self.profile is not None else None)

    def serve_spans_device(self, trace_begin: int, n_traces: int, d_records: int, d_stats: int, d_table: int,
                           d_workspace: int, workspace_bytes: int, tap=None, stream: int = 0,
                           wide: bool = False) -> None:
        """isim_serve_des_spans_device: the batch of serve_device, and after it the spans of the traces `tap`
        (a native.DesTap over device addresses, isim.des_spans.make_tap) chooses.  tap None: serve_device."""
        p, lp = self._load_args(wide)
        native.check(native.load().isim_serve_des_spans_device(
            self.handler._h, C.byref(p), lp, trace_begin, n_traces, d_records or None, d_stats, d_table,
            d_workspace, workspace_bytes, C.byref(tap) if tap is not None else None, stream or None))

    def serve_spans(self, trace_begin: int, n_traces: int, q_ppm: int = 999000, min_latency_ns: int = None,
                    cls: int = native.Q_ALL, max_traces: int = 64, cap_spans: int = 2 ** 20, wide: bool = False,
                    device: int = 0, wait_table=None, critical_path: bool = False):
        """Synchronous: (records, stats, DES table, [DesTrace], DesWaitTable) of one batch.  The traces: the
        records at or above the batch's q_ppm order statistic (p99.9) in class cls, or at or above
        min_latency_ns when that is given; ids ascending, the first max_traces whose spans fit cap_spans.
        wait_table: a DesWaitTable to add into (a new one otherwise).  critical_path: a DesCriticalPath of
        those traces is appended to the tuple, folded on the device on the batch's stream before the copy
        back (the traces' critical spans are marked).  Item engine only."""
        from .des_spans import DES_SPAN_DTYPE, DesTrace, DesWaitTable, make_tap
        from .sim import REC_DTYPE as _REC
        names = [s["name"] for s in self.handler.graph.canonical()["services"]]
        waits = wait_table if wait_table is not None else DesWaitTable(self.handler, names=names)
        if critical_path:
            return self._serve_spans_critical(trace_begin, n_traces, 0 if min_latency_ns is None else min_latency_ns,
                                              q_ppm if min_latency_ns is None else 0, cls, max_traces, cap_spans,
                                              wide, device, waits, names)
        n_ids = min(int(max_traces), int(n_traces))
        ids, off = np.zeros(max(1, n_ids), np.uint64), np.zeros(n_ids + 1, np.uint64)
        spans = np.zeros(max(1, int(cap_spans)), DES_SPAN_DTYPE)
        info = np.zeros(native.DES_SPAN_INFO_WORDS, np.uint64)
        tap = make_tap(0 if min_latency_ns is None else min_latency_ns, q_ppm if min_latency_ns is None else 0, cls,
                       max_traces, cap_spans, ids.ctypes.data, off.ctypes.data, spans.ctypes.data, info.ctypes.data,
                       waits.table.ctypes.data)
        stats, table = self.handler.new_stats(), self.new_table()
        recs = np.zeros(n_traces, _REC)
        p, lp = self._load_args(wide)
        native.check(native.load().isim_serve_des_spans(
            self.handler._h, device, C.byref(p), lp, trace_begin, n_traces, recs.ctypes.data if n_traces else None,
            stats.ctypes.data, table.ctypes.data, C.byref(tap)))
        written = int(info[native.SPAN_WRITTEN])
        traces = [DesTrace(ids[i], spans[int(off[i]):int(off[i + 1])].copy(), names) for i in range(written)]
        self.last_tap_info = info
        return recs, stats, table, traces, waits

    def _serve_spans_critical(self, trace_begin, n_traces, min_latency_ns, q_ppm, cls, max_traces, cap_spans, wide,
                              device, waits, names):
        """serve_spans with the DES critical path: device buffers, the batch with its tap and the fold on one
        stream, then one copy back.  32-bit rows first, and again wide if the batch asks for it."""
        import torch
        from . import des_spans as ds
        from .sim import REC_DTYPE as _REC
        n_ids = min(int(max_traces), int(n_traces))
        cap_spans = int(cap_spans)
        dev = torch.device("cuda", device)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            z = lambda n: torch.zeros(max(1, n), dtype=torch.int64, device=dev)  # noqa: E731
            ws = z(self.workspace_bytes(n_traces) // 8 + 1)
            cws = z(ds.critical_path_workspace_bytes(self.handler, cap_spans) // 8)
            for w in ([False, True] if not wide else [True]):
                stats, table, rec = z(len(self.handler.new_stats())), z(self.table_words), z(2 * n_traces)
                ids, off, spans, info = z(n_ids), z(n_ids + 1), z(8 * cap_spans), z(native.DES_SPAN_INFO_WORDS)
                wt = torch.from_numpy(waits.table.view(np.int64).ravel().copy()).to(dev)
                cpt, tw = z(ds.critical_path_table_words(self.handler)), z(n_ids)
                tap = ds.make_tap(min_latency_ns, q_ppm, cls, n_ids, cap_spans, ids.data_ptr(), off.data_ptr(),
                                  spans.data_ptr(), info.data_ptr(), wt.data_ptr())
                self.serve_spans_device(trace_begin, n_traces, rec.data_ptr() if n_traces else 0, stats.data_ptr(),
                                        table.data_ptr(), ws.data_ptr(), ws.numel() * 8, tap, stream, wide=w)
                ds.des_critical_path_device(self.handler, off.data_ptr(), spans.data_ptr(), cap_spans, info.data_ptr(),
                                            n_ids, cpt.data_ptr(), tw.data_ptr(), cws.data_ptr(), cws.numel() * 8, stream)
                h_stats = u64(stats)[:len(self.handler.new_stats())]
                if not int(h_stats[native.ST_DES_RETRY]):
                    break
            h_info, h_off, h_ids = u64(info), u64(off), u64(ids)
            written = int(h_info[native.SPAN_WRITTEN])
            h_spans = spans[:8 * int(h_off[written])].cpu().numpy().view(ds.DES_SPAN_DTYPE)
            waits.table[...] = u64(wt).reshape(waits.table.shape)
            path = ds.DesCriticalPath(self.handler, u64(cpt)[:ds.critical_path_table_words(self.handler)], names,
                                      u64(tw)[:written].copy())
            recs = rec[:2 * n_traces].cpu().numpy().view(_REC)
            h_table = u64(table)[:max(1, self.table_words)].copy()
        traces = [ds.DesTrace(h_ids[i], h_spans[int(h_off[i]):int(h_off[i + 1])].copy(), names) for i in range(written)]
        self.last_tap_info = h_info
        return recs, h_stats.copy(), h_table, traces, waits, path

    def service_timeline(self, trace_begin: int, n_traces: int, window_ns: int, n_windows: int, t0_ns: int = 0,
                         device: int = 0, into=None, cap_spans: int = None):
        """The ServiceTimeline of one batch: the whole batch tapped (threshold 0, every trace,
        room for hops_upper spans per trace unless cap_spans says otherwise) and folded on the same stream;
        only the table comes back.  into: a ServiceTimeline of the same parameters to add into (a new one
        otherwise).  32-bit rows first, and again wide if the batch asks for it.  Raises if the spans did
        not fit cap_spans: never a partial table.  Item engine only."""
        import torch
        from . import des_spans as ds
        from .service_timeline import (ServiceTimeline, service_timeline_device,
                                       service_timeline_workspace_bytes)
        if into is None:
            into = ServiceTimeline(self.handler, window_ns, n_windows, t0_ns)
        elif (into.window_ns, into.n_windows, into.t0_ns) != (int(window_ns), int(n_windows), int(t0_ns)):
            raise ValueError("`into` has other timeline parameters")
        n_traces = int(n_traces)
        cap = n_traces * int(self.handler.info.hops_upper) if cap_spans is None else int(cap_spans)
        dev = torch.device("cuda", device)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            z = lambda n: torch.zeros(max(1, n), dtype=torch.int64, device=dev)  # noqa: E731
            ws = z(self.workspace_bytes(n_traces) // 8 + 1)
            tws = z(service_timeline_workspace_bytes(self.handler, window_ns, n_windows, t0_ns) // 8)
            for w in [False, True]:
                stats, table, rec = z(len(self.handler.new_stats())), z(self.table_words), z(2 * n_traces)
                ids, off, spans, info = z(n_traces), z(n_traces + 1), z(8 * cap), z(native.DES_SPAN_INFO_WORDS)
                out = torch.from_numpy(into.flat.view(np.int64).copy()).to(dev)
                tap = ds.make_tap(0, 0, native.Q_ALL, n_traces, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(),
                                  info.data_ptr())
                self.serve_spans_device(trace_begin, n_traces, rec.data_ptr() if n_traces else 0, stats.data_ptr(),
                                        table.data_ptr(), ws.data_ptr(), ws.numel() * 8, tap, stream, wide=w)
                service_timeline_device(self.handler, window_ns, n_windows, t0_ns, off.data_ptr(),
                                            spans.data_ptr(), cap, info.data_ptr(), out.data_ptr(), tws.data_ptr(),
                                            tws.numel() * 8, stream)
                if not int(u64(stats)[native.ST_DES_RETRY]):
                    break
            h_info = u64(info)
            h_out = u64(out)
        self.last_tap_info = h_info
        if int(h_info[native.DES_SPAN_MATCHES]) != int(h_info[native.SPAN_WRITTEN]):
            raise RuntimeError(f"service_timeline: the batch has {int(h_info[native.SPAN_TOTAL])} spans, cap_spans "
                               f"{cap} holds {int(h_info[native.SPAN_WRITTEN])} of its "
                               f"{int(h_info[native.DES_SPAN_MATCHES])} traces")
        into.flat[...] = h_out[:into.flat.size]
        return into

    def service_quantiles(self, trace_begin: int, n_traces: int, q=DEFAULT_Q, device: int = 0, cap_spans: int = None):
        """The ServiceQuantiles of one batch: the whole batch tapped as service_timeline taps
        it and the per-service select made on the same stream; only the table comes back.  32-bit rows
        first, and again wide if the batch asks for it.  Raises if the spans did not fit cap_spans: never a
        partial table.  Item engine only."""
        import torch
        from . import des_spans as ds
        from .service_quantiles import (ServiceQuantiles, service_quantiles_device, service_quantiles_table_words,
                                        service_quantiles_workspace_bytes)
        q = tuple(q)
        n_traces = int(n_traces)
        cap = n_traces * int(self.handler.info.hops_upper) if cap_spans is None else int(cap_spans)
        words = service_quantiles_table_words(self.handler, len(q))
        qws_bytes = service_quantiles_workspace_bytes(self.handler, cap, len(q))
        dev = torch.device("cuda", device)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            z = lambda n: torch.zeros(max(1, n), dtype=torch.int64, device=dev)  # noqa: E731
            ws = z(self.workspace_bytes(n_traces) // 8 + 1)
            qws = torch.empty(max(1, qws_bytes // 8 + 1), dtype=torch.int64, device=dev)
            out = torch.empty(words, dtype=torch.int64, device=dev)
            for w in [False, True]:
                stats, table, rec = z(len(self.handler.new_stats())), z(self.table_words), z(2 * n_traces)
                ids, off, spans, info = z(n_traces), z(n_traces + 1), z(8 * cap), z(native.DES_SPAN_INFO_WORDS)
                tap = ds.make_tap(0, 0, native.Q_ALL, n_traces, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(),
                                  info.data_ptr())
                self.serve_spans_device(trace_begin, n_traces, rec.data_ptr() if n_traces else 0, stats.data_ptr(),
                                        table.data_ptr(), ws.data_ptr(), ws.numel() * 8, tap, stream, wide=w)
                service_quantiles_device(self.handler, q, off.data_ptr(), spans.data_ptr(), cap, info.data_ptr(),
                                         out.data_ptr(), qws.data_ptr(), qws.numel() * 8, stream)
                if not int(u64(stats)[native.ST_DES_RETRY]):
                    break
            h_info = u64(info)
            h_out = u64(out)
        self.last_tap_info = h_info
        if int(h_info[native.DES_SPAN_MATCHES]) != int(h_info[native.SPAN_WRITTEN]):
            raise RuntimeError(f"service_quantiles: the batch has {int(h_info[native.SPAN_TOTAL])} spans, cap_spans "
                               f"{cap} holds {int(h_info[native.SPAN_WRITTEN])} of its "
                               f"{int(h_info[native.DES_SPAN_MATCHES])} traces")
        return ServiceQuantiles(self.handler, q, h_out[:words].copy())

    def service_sketch(self, trace_begin: int, n_traces: int, sub_bits: int = 3, device: int = 0, into=None,
                       cap_spans: int = None):
        """The ServiceSketch of one batch, added into `into` (a ServiceSketch of this handler
        and sub_bits; a new one if None) and returned: the whole batch tapped as service_quantiles taps it
        and sketched on the same stream; only the batch's table comes back.  32-bit rows first, and again
        wide if the batch asks for it (the first attempt wrote no span and added nothing).  Raises if the
        spans did not fit cap_spans, and then `into` is unchanged.  Item engine only."""
        import torch
        from . import des_spans as ds
        from .service_sketch import (ServiceSketch, service_sketch_device, service_sketch_table_words,
                                     service_sketch_workspace_bytes)
        n_traces = int(n_traces)
        if into is not None and (into.sub_bits != int(sub_bits) or into.handler is not self.handler):
            raise ValueError("service_sketch: `into` is a sketch of another handler or sub_bits")
        cap = n_traces * int(self.handler.info.hops_upper) if cap_spans is None else int(cap_spans)
        words = service_sketch_table_words(self.handler, sub_bits)
        kws_bytes = service_sketch_workspace_bytes(self.handler, cap)
        dev = torch.device("cuda", device)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            z = lambda n: torch.zeros(max(1, n), dtype=torch.int64, device=dev)  # noqa: E731
            ws = z(self.workspace_bytes(n_traces) // 8 + 1)
            kws = torch.empty(max(1, kws_bytes // 8 + 1), dtype=torch.int64, device=dev)
            for w in [False, True]:
                out = z(words)  # this attempt's own table: a retried attempt leaves nothing behind
                stats, table, rec = z(len(self.handler.new_stats())), z(self.table_words), z(2 * n_traces)
                ids, off, spans, info = z(n_traces), z(n_traces + 1), z(8 * cap), z(native.DES_SPAN_INFO_WORDS)
                tap = ds.make_tap(0, 0, native.Q_ALL, n_traces, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(),
                                  info.data_ptr())
                self.serve_spans_device(trace_begin, n_traces, rec.data_ptr() if n_traces else 0, stats.data_ptr(),
                                        table.data_ptr(), ws.data_ptr(), ws.numel() * 8, tap, stream, wide=w)
                service_sketch_device(self.handler, sub_bits, off.data_ptr(), spans.data_ptr(), cap, info.data_ptr(),
                                      out.data_ptr(), kws.data_ptr(), kws.numel() * 8, stream)
                if not int(u64(stats)[native.ST_DES_RETRY]):
                    break
            h_info = u64(info)
            h_out = u64(out)
        self.last_tap_info = h_info
        if int(h_info[native.DES_SPAN_MATCHES]) != int(h_info[native.SPAN_WRITTEN]):
            raise RuntimeError(f"service_sketch: the batch has {int(h_info[native.SPAN_TOTAL])} spans, cap_spans "
                               f"{cap} holds {int(h_info[native.SPAN_WRITTEN])} of its "
                               f"{int(h_info[native.DES_SPAN_MATCHES])} traces")
        batch = ServiceSketch(self.handler, sub_bits, h_out[:words].copy())
        return batch if into is None else into.merge(batch)

    def service_window_quantiles(self, trace_begin: int, n_traces: int, q=DEFAULT_Q, window_ns: int = 1_000_000,
                                 n_windows: int = 100, t0_ns: int = 0, device: int = 0, cap_spans: int = None):
        """The ServiceWindowQuantiles of one batch: the whole batch tapped as service_timeline
        taps it, its windows given as service_timeline takes them, and the select per (service, row) made on
        the same stream; only the table comes back.  32-bit rows first, and again wide if the batch asks for
        it.  Raises if the spans did not fit cap_spans: never a partial table.  Item engine only."""
        import torch
        from . import des_spans as ds
        from .service_window_quantiles import (ServiceWindowQuantiles, service_window_quantiles_device,
                                               service_window_quantiles_table_words,
                                               service_window_quantiles_workspace_bytes)
        q = tuple(q)
        n_traces = int(n_traces)
        cap = n_traces * int(self.handler.info.hops_upper) if cap_spans is None else int(cap_spans)
        words = service_window_quantiles_table_words(self.handler, len(q), window_ns, n_windows, t0_ns)
        qws_bytes = service_window_quantiles_workspace_bytes(self.handler, cap, len(q), window_ns, n_windows, t0_ns)
        dev = torch.device("cuda", device)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            z = lambda n: torch.zeros(max(1, n), dtype=torch.int64, device=dev)  # noqa: E731
            ws = z(self.workspace_bytes(n_traces) // 8 + 1)
            qws = torch.empty(max(1, qws_bytes // 8 + 1), dtype=torch.int64, device=dev)
            out = torch.empty(words, dtype=torch.int64, device=dev)
            for w in [False, True]:
                stats, table, rec = z(len(self.handler.new_stats())), z(self.table_words), z(2 * n_traces)
                ids, off, spans, info = z(n_traces), z(n_traces + 1), z(8 * cap), z(native.DES_SPAN_INFO_WORDS)
                tap = ds.make_tap(0, 0, native.Q_ALL, n_traces, cap, ids.data_ptr(), off.data_ptr(), spans.data_ptr(),
                                  info.data_ptr())
                self.serve_spans_device(trace_begin, n_traces, rec.data_ptr() if n_traces else 0, stats.data_ptr(),
                                        table.data_ptr(), ws.data_ptr(), ws.numel() * 8, tap, stream, wide=w)
                service_window_quantiles_device(self.handler, q, window_ns, n_windows, t0_ns, off.data_ptr(),
                                                spans.data_ptr(), cap, info.data_ptr(), out.data_ptr(),
                                                qws.data_ptr(), qws.numel() * 8, stream)
                if not int(u64(stats)[native.ST_DES_RETRY]):
                    break
            h_info = u64(info)
            h_out = u64(out)
        self.last_tap_info = h_info
        if int(h_info[native.DES_SPAN_MATCHES]) != int(h_info[native.SPAN_WRITTEN]):
            raise RuntimeError(f"service_window_quantiles: the batch has {int(h_info[native.SPAN_TOTAL])} spans, "
                               f"cap_spans {cap} holds {int(h_info[native.SPAN_WRITTEN])} of its "
                               f"{int(h_info[native.DES_SPAN_MATCHES])} traces")
        return ServiceWindowQuantiles(self.handler, q, window_ns, n_windows, t0_ns, h_out[:words].copy())

    def arrivals(self, trace_begin: int, n_traces: int, device: int = 0) -> np.ndarray:
        """The arrival times (u64 ns since batch start) `serve` uses for these traces."""
        if self.profile is not None:
            from .load_profile import profile_arrivals
            return profile_arrivals(self.handler, self.profile, trace_begin, n_traces, device)
        from .timeline import des_arrivals
        return des_arrivals(self.handler, self.params.mean_interarrival_ns, trace_begin, n_traces, device)

    def timeline(self, trace_begin: int, n_traces: int, window_ns: int, n_windows: int, t0_ns: int = 0,
                 device: int = 0) -> dict:
        """Serves the batch (as `serve`: wide rows on retry) and bins it into
        windows of simulated time: isim.timeline of its arrivals and records."""
        from .timeline import timeline
        recs, _, _ = self.serve(trace_begin, n_traces, device)
        return timeline(self.arrivals(trace_begin, n_traces, device), recs, window_ns, n_windows, t0_ns, device)

    def timeline_quantiles(self, trace_begin: int, n_traces: int, window_ns: int, n_windows: int, t0_ns: int = 0,
                           q=DEFAULT_Q, device: int = 0) -> dict:
        """Serves the batch (as `serve`) and gives the exact latency percentiles of what
        completes in each window: isim.timeline_quantiles of its arrivals and records."""
        from .timeline_quantiles import timeline_quantiles
        recs, _, _ = self.serve(trace_begin, n_traces, device)
        return timeline_quantiles(self.arrivals(trace_begin, n_traces, device), recs, window_ns, n_windows, t0_ns,
                                  q, device)

    def timeline_sketch(self, trace_begin: int, n_traces: int, window_ns: int, n_windows: int, t0_ns: int = 0,
                        sub_bits: int = 7, q=DEFAULT_Q, device: int = 0) -> dict:
        """Serves the batch (as `serve`) and gives per window the mergeable latency sketch of what
        completes in it, with its quantile brackets: isim.timeline_sketch of its arrivals and records."""
        from .sketch import timeline_sketch
        recs, _, _ = self.serve(trace_begin, n_traces, device)
        return timeline_sketch(self.arrivals(trace_begin, n_traces, device), recs, window_ns, n_windows, t0_ns,
                               sub_bits, q, device)

    def fold(self, table: np.ndarray) -> np.ndarray:
        n = self.handler.info.n_services
        out = np.zeros((max(1, n), native.DES_ROW_WORDS), np.uint64)
        table = np.ascontiguousarray(table, dtype=np.uint64)
        native.check(native.load().isim_des_fold(self.handler._h, table.ctypes.data, out.ctypes.data))
        return out[:n]
