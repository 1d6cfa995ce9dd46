// Package isim runs isotope service-graph scripts for many request traces on
// an MI355X through libisim (include/isim.h): the cgo binding a maintainer
// adds next to isotope/service/pkg/srv (graph.go:34 HandlerFromServiceGraphYAML,
// handler.go:37 ServeHTTP) and isotope/convert/pkg (graph decoding, graphviz,
// kubernetes).  Build: make -C istio-isotope_amd/csrc (libisim.so), then
// `go build ./...` in go/ (needs a Go toolchain and sigs.k8s.io/yaml v1.2.0,
// the reference's own pin, isotope/go.mod:17).
package isim

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../istio-isotope_amd/isim -lisim -Wl,-rpath,${SRCDIR}/../../istio-isotope_amd/isim
#include <stdlib.h>
#include "isim.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"unsafe"

	"sigs.k8s.io/yaml"
)

type Graph struct{ g *C.isim_graph }
type Handler struct{ h *C.isim_handler }
type Params = C.isim_params
type TraceRecord = C.isim_trace_rec

func lastErr(rc C.int) error {
	if rc == C.ISIM_OK {
		return nil
	}
	return fmt.Errorf("isim status %d: %s", int(rc), C.GoString(C.isim_last_error()))
}

// GraphFromYAML mirrors yaml.Unmarshal(bytes, &graph.ServiceGraph{}):
// sigs.k8s.io/yaml converts to JSON, libisim applies UnmarshalJSON.
func GraphFromYAML(b []byte) (*Graph, error) {
	j, err := yaml.YAMLToJSON(b)
	if err != nil {
		return nil, err
	}
	if len(j) == 0 {
		return nil, errors.New("empty graph")
	}
	var g *C.isim_graph
	rc := C.isim_graph_unmarshal_json((*C.char)(unsafe.Pointer(&j[0])), C.size_t(len(j)), &g)
	if rc != C.ISIM_OK {
		return nil, lastErr(rc)
	}
	return &Graph{g}, nil
}

func (g *Graph) Close() { C.isim_graph_free(g.g) }

// NewHandler mirrors srv.HandlerFromServiceGraphYAML(path, serviceName);
// serviceName "" selects the first isEntrypoint service.
func NewHandler(g *Graph, serviceName string, p Params) (*Handler, error) {
	var name *C.char
	if serviceName != "" {
		name = C.CString(serviceName)
		defer C.free(unsafe.Pointer(name))
	}
	var h *C.isim_handler
	if rc := C.isim_handler_create(g.g, name, &p, &h); rc != C.ISIM_OK {
		return nil, lastErr(rc)
	}
	return &Handler{h}, nil
}

// Serve simulates traces [begin, begin+len(recs)) on GPU `device`; stats is
// resized to the handler's stats words.
func (h *Handler) Serve(device int, begin uint64, recs []TraceRecord) ([]uint64, error) {
	var info C.isim_handler_info
	if rc := C.isim_handler_info_get(h.h, &info); rc != C.ISIM_OK {
		return nil, lastErr(rc)
	}
	stats := make([]uint64, int(info.stats_words))
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	rc := C.isim_serve(h.h, C.int(device), C.uint64_t(begin), C.uint64_t(len(recs)), rp,
		u64ptr(stats))
	return stats, lastErr(rc)
}

func (h *Handler) Close() { C.isim_handler_free(h.h) }

// MarshalJSON returns json.Marshal(graph) as Go would produce it; DOT the
// `isotope convert graphviz` text.
func (g *Graph) text(f func(*C.isim_graph, *C.char, C.size_t, *C.size_t) C.int) (string, error) {
	var n C.size_t
	if rc := f(g.g, nil, 0, &n); rc != C.ISIM_OK {
		return "", lastErr(rc)
	}
	buf := make([]byte, int(n))
	if rc := f(g.g, (*C.char)(unsafe.Pointer(&buf[0])), n, &n); rc != C.ISIM_OK {
		return "", lastErr(rc)
	}
	return string(buf[:len(buf)-1]), nil
}
func (g *Graph) MarshalJSON() ([]byte, error) {
	s, err := g.text(func(a *C.isim_graph, b *C.char, c C.size_t, d *C.size_t) C.int {
		return C.isim_graph_marshal_json(a, b, c, d)
	})
	return []byte(s), err
}
func (g *Graph) DOT() (string, error) {
	return g.text(func(a *C.isim_graph, b *C.char, c C.size_t, d *C.size_t) C.int {
		return C.isim_graph_to_dot(a, b, c, d)
	})
}

// ServeUnderLoad runs the per-replica worker-pool DES (config 5) for
// len(recs) open-loop arrivals with the given mean gap.
func (h *Handler) ServeUnderLoad(device int, begin uint64, meanGapNs uint64, recs []TraceRecord) (stats, table []uint64, err error) {
	var info C.isim_handler_info
	var dinfo C.isim_des_info
	if rc := C.isim_handler_info_get(h.h, &info); rc != C.ISIM_OK {
		return nil, nil, lastErr(rc)
	}
	if rc := C.isim_des_info_get(h.h, &dinfo); rc != C.ISIM_OK {
		return nil, nil, lastErr(rc) // outside the DES graph class: the reason is in the message
	}
	stats = make([]uint64, int(info.stats_words))
	table = make([]uint64, int(dinfo.table_rows)*C.ISIM_DES_ROW_WORDS+1)
	p := C.isim_des_params{mean_interarrival_ns: C.uint64_t(meanGapNs)}
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	// 32-bit rows; a batch with a latency >= 2^31 ns is rerun with 64-bit rows inside the call
	rc := C.isim_serve_des(h.h, C.int(device), &p, C.uint64_t(begin), C.uint64_t(len(recs)), rp,
		u64ptr(stats), u64ptr(table))
	return stats, table, lastErr(rc)
}

// DesBatch is the item engine's report on the handler's last DES batch
// (isim_des_last_batch): passes over the rounds, host synchronisations,
// executed invocations.
type DesBatch struct {
	Passes, Syncs uint32
	Items         uint64
}

// LastDesBatch reports the item engine's last batch (zero before the first).
func (h *Handler) LastDesBatch() (DesBatch, error) {
	var st C.isim_des_batch_stats
	if rc := C.isim_des_last_batch(h.h, &st); rc != C.ISIM_OK {
		return DesBatch{}, lastErr(rc)
	}
	return DesBatch{uint32(st.passes), uint32(st.syncs), uint64(st.items)}, nil
}

// SetDesWorkers sets the workers per replica of every service, by service
// index (isim_des_workers_set): 1 .. 65536 each, behind the replica's one FIFO
// queue.  nil resets every service to 1.  Handler state, read at the start of
// each DES batch; not to be changed while one is in flight.  More than one
// worker needs the item engine (ISIM_FLAG_DYNAMIC) and an acyclic call-step
// schedule.
func (h *Handler) SetDesWorkers(workers []uint32) error {
	var wp *C.uint32_t
	if len(workers) > 0 {
		wp = (*C.uint32_t)(unsafe.Pointer(&workers[0]))
	}
	return lastErr(C.isim_des_workers_set(h.h, wp, C.uint32_t(len(workers))))
}

// DesWorkers returns the workers per replica of the nServices services
// (isim_des_workers_get): 1 each until set.
func (h *Handler) DesWorkers(nServices int) ([]uint32, error) {
	w := make([]uint32, nServices+1)
	if err := lastErr(C.isim_des_workers_get(h.h, (*C.uint32_t)(unsafe.Pointer(&w[0])))); err != nil {
		return nil, err
	}
	return w[:nServices], nil
}

// Quantiles is one class's exact latency percentiles (isim_latency_quantiles):
// the records in the class and, per requested quantile, the nearest-rank
// latency in ns (all 0 for an empty class).
type Quantiles struct {
	Count  uint64
	Values []uint64
}

// LatencyQuantiles computes exact percentiles of recs' latencies on GPU
// `device`, for every record, the 200s and the 500s (C.ISIM_Q_ALL /
// ISIM_Q_200 / ISIM_Q_500).  qPpm are parts per million (p99.9 = 999000), at
// most C.ISIM_MAX_QUANTILES of them, in any order.
func LatencyQuantiles(device int, recs []TraceRecord, qPpm []uint32) ([3]Quantiles, error) {
	var res [3]Quantiles
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	var qp *C.uint32_t
	if len(qPpm) > 0 {
		qp = (*C.uint32_t)(unsafe.Pointer(&qPpm[0]))
	}
	nq := len(qPpm)
	if nq < 1 || nq > C.ISIM_MAX_QUANTILES {
		// libisim's EINVAL and message; the output is never written
		return res, lastErr(C.isim_latency_quantiles(C.int(device), rp, C.uint64_t(len(recs)), qp, C.uint32_t(nq), nil))
	}
	out := make([]uint64, 3*(1+nq)) // ISIM_Q_OUT_WORDS (cgo sees no function-like macros)
	rc := C.isim_latency_quantiles(C.int(device), rp, C.uint64_t(len(recs)), qp, C.uint32_t(nq), u64ptr(out))
	if rc != C.ISIM_OK {
		return res, lastErr(rc)
	}
	for c := range res {
		row := out[c*(1+nq) : (c+1)*(1+nq)]
		res[c] = Quantiles{Count: row[0], Values: row[1:]}
	}
	return res, nil
}

// DesArrivals returns the arrival times (ns since batch start) ServeUnderLoad
// uses for traces [begin, begin+n) at the same mean gap (isim_des_arrivals).
func (h *Handler) DesArrivals(device int, begin uint64, meanGapNs uint64, n int) ([]uint64, error) {
	p := C.isim_des_params{mean_interarrival_ns: C.uint64_t(meanGapNs)}
	out := make([]uint64, n)
	rc := C.isim_des_arrivals(h.h, C.int(device), &p, C.uint64_t(begin), C.uint64_t(n), u64ptr(out))
	return out, lastErr(rc)
}

// ClosedLoop is the reference's load client (Fortio's connections and qps):
// each of Connections sends its next request when the previous response has
// arrived and, with PeriodNs > 0, not before its slot (isim.h, DESIGN §18).
type ClosedLoop struct {
	Connections uint32
	PeriodNs    uint64 // per connection; 0 is qps "max"
	Uniform     bool   // stagger the connections' slots (Fortio's -uniform)
}

// ClosedLoopInfo is the info block of a closed-loop batch.
type ClosedLoopInfo struct {
	MakespanNs, MinFreeNs, Late, SumLateNs uint64
}

func (c ClosedLoop) batch(recs []TraceRecord, firstIndex uint64, freeAt []uint64,
	call func(*C.struct_isim_closed_loop, *TraceRecord, *C.uint64_t, *C.uint64_t, *C.uint64_t) C.int) ([]uint64, ClosedLoopInfo, error) {
	if freeAt != nil && len(freeAt) != int(c.Connections) {
		return nil, ClosedLoopInfo{}, errors.New("freeAt must hold one value per connection")
	}
	p := C.struct_isim_closed_loop{connections: C.uint32_t(c.Connections), period_ns: C.uint64_t(c.PeriodNs),
		first_index: C.uint64_t(firstIndex)}
	if c.Uniform {
		p.flags = C.ISIM_CL_UNIFORM
	}
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	arrivals := make([]uint64, len(recs))
	info := make([]uint64, C.ISIM_CL_INFO_WORDS)
	rc := call(&p, rp, u64ptr(freeAt), u64ptr(arrivals), u64ptr(info))
	return arrivals, ClosedLoopInfo{info[C.ISIM_CL_MAKESPAN], info[C.ISIM_CL_MIN_FREE], info[C.ISIM_CL_LATE],
		info[C.ISIM_CL_SUM_LATE]}, lastErr(rc)
}

// Arrivals returns the arrival times of recs as requests firstIndex.. of the
// run, on GPU `device` (isim_closed_loop).  freeAt, one value per connection,
// is read and overwritten with the state after the batch; nil starts a run
// and returns no state.
func (c ClosedLoop) Arrivals(device int, recs []TraceRecord, firstIndex uint64, freeAt []uint64) ([]uint64, ClosedLoopInfo, error) {
	return c.batch(recs, firstIndex, freeAt, func(p *C.struct_isim_closed_loop, r *TraceRecord, f, a, i *C.uint64_t) C.int {
		return C.isim_closed_loop(C.int(device), p, r, C.uint64_t(len(recs)), f, a, i)
	})
}

// ArrivalsHost is Arrivals on the host, without a GPU (isim_closed_loop_host).
func (c ClosedLoop) ArrivalsHost(recs []TraceRecord, firstIndex uint64, freeAt []uint64) ([]uint64, ClosedLoopInfo, error) {
	return c.batch(recs, firstIndex, freeAt, func(p *C.struct_isim_closed_loop, r *TraceRecord, f, a, i *C.uint64_t) C.int {
		return C.isim_closed_loop_host(p, r, C.uint64_t(len(recs)), f, a, i)
	})
}

// Span is one executed invocation of a trace (isim_span, DESIGN §19): the call
// occupies [StartNs, StartNs + HopNs + DurationNs] of the trace's time.
type Span = C.isim_span

// TraceSpans walks the listed traces again on GPU `device` and returns, per
// trace, its executed invocations in hop order with their start times
// (isim_trace_spans).  The handler must run a dynamic walk over an unrolled
// tree (or be created with ISIM_FLAG_DYNAMIC).
func (h *Handler) TraceSpans(device int, ids []uint64) ([][]Span, error) {
	off := make([]uint64, len(ids)+1)
	info := make([]uint64, C.ISIM_SPAN_INFO_WORDS)
	// no room first: the call then only counts, and info tells the room the traces need
	rc := C.isim_trace_spans(C.int(device), h.h, u64ptr(ids), C.uint64_t(len(ids)), u64ptr(off), nil, 0, u64ptr(info))
	if err := lastErr(rc); err != nil {
		return nil, err
	}
	spans := make([]Span, info[C.ISIM_SPAN_TOTAL]+1)
	rc = C.isim_trace_spans(C.int(device), h.h, u64ptr(ids), C.uint64_t(len(ids)), u64ptr(off), &spans[0],
		C.uint64_t(info[C.ISIM_SPAN_TOTAL]), u64ptr(info))
	if err := lastErr(rc); err != nil {
		return nil, err
	}
	out := make([][]Span, len(ids))
	for i := range ids {
		out[i] = spans[off[i]:off[i+1]]
	}
	return out, nil
}

// The critical-path table (DESIGN §20): (services + 1) rows of CpRowWords
// words, every word a sum mod 2^64 (tables merge by addition).  Row s holds
// the Cp* words of service s, the last row the CpH* words.  SpanCritical is
// the status bit of a span on the path.
const (
	SpanCritical  = C.ISIM_SPAN_CRITICAL
	CpInvocations = C.ISIM_CP_INVOCATIONS
	CpSumDuration = C.ISIM_CP_SUM_DURATION
	CpCritical    = C.ISIM_CP_CRITICAL
	CpSelfNs      = C.ISIM_CP_SELF_NS
	CpHopNs       = C.ISIM_CP_HOP_NS
	CpCritical500 = C.ISIM_CP_CRITICAL_500
	CpRowWords    = C.ISIM_CP_ROW_WORDS
	CpHTraces     = C.ISIM_CP_H_TRACES
	CpHSpans      = C.ISIM_CP_H_SPANS
	CpHCritical   = C.ISIM_CP_H_CRITICAL
	CpHSumLatency = C.ISIM_CP_H_SUM_LATENCY
	CpHRefused    = C.ISIM_CP_H_REFUSED
)

// CriticalPath walks the listed traces again on GPU `device`, marks the spans
// on each trace's critical path (SpanCritical in Span.status) and returns them
// with the table of per-service time on the path (isim_trace_spans, then
// isim_critical_path).  Tables of several calls add word by word.
func (h *Handler) CriticalPath(device int, ids []uint64) ([][]Span, []uint64, error) {
	var words C.uint64_t
	if err := lastErr(C.isim_critical_path_table_words(h.h, &words)); err != nil {
		return nil, nil, err
	}
	traces, err := h.TraceSpans(device, ids)
	if err != nil {
		return nil, nil, err
	}
	// TraceSpans returns slices of one array, in list order: the offsets are their running lengths
	off := make([]uint64, len(ids)+1)
	for i, t := range traces {
		off[i+1] = off[i] + uint64(len(t))
	}
	table := make([]uint64, words)
	var first *Span
	if len(traces) > 0 {
		first = &traces[0][0] // every trace has its entry span
	}
	rc := C.isim_critical_path(C.int(device), h.h, u64ptr(off), C.uint64_t(len(ids)), first, u64ptr(table))
	if err := lastErr(rc); err != nil {
		return nil, nil, err
	}
	return traces, table, nil
}

// DesSpan is one executed invocation of a trace of a DES batch (isim_des_span,
// DESIGN §21): it reached its replica's queue at arrival_ns, the worker took it
// at start_ns and it responded at finish_ns, all on the batch clock.
type DesSpan = C.isim_des_span

// The DES wait table (DESIGN §21): (services + 1) rows of DwRowWords words over
// the emitted spans; tables merge by addition except DwMaxWait (DesWaitMerge).
const (
	DesSpanMatches = C.ISIM_DES_SPAN_MATCHES
	DwInvocations  = C.ISIM_DW_INVOCATIONS
	DwWaited       = C.ISIM_DW_WAITED
	DwSumWait      = C.ISIM_DW_SUM_WAIT
	DwMaxWait      = C.ISIM_DW_MAX_WAIT
	DwSumDuration  = C.ISIM_DW_SUM_DURATION
	DwResp500      = C.ISIM_DW_RESP_500
	DwRowWords     = C.ISIM_DW_ROW_WORDS
	DwHTraces      = C.ISIM_DW_H_TRACES
	DwHSpans       = C.ISIM_DW_H_SPANS
	DwHSumLatency  = C.ISIM_DW_H_SUM_LATENCY
	DwHSumWait     = C.ISIM_DW_H_SUM_WAIT
)

// ServeDesSpans runs one DES batch under the constant mean gap meanNs on GPU
// `device` and returns its records and, for the traces at or above the batch's
// qPpm order statistic (at most maxTraces whose spans fit capSpans), their
// invocations with queue times, and the wait table (isim_serve_des_spans).  The
// handler's DES must run on the item engine (ISIM_FLAG_DYNAMIC).
func (h *Handler) ServeDesSpans(device int, meanNs, begin uint64, n int, qPpm uint32, maxTraces, capSpans int) ([]TraceRecord, [][]DesSpan, []uint64, error) {
	var words C.uint64_t
	if err := lastErr(C.isim_des_wait_table_words(h.h, &words)); err != nil {
		return nil, nil, nil, err
	}
	if maxTraces > n {
		maxTraces = n
	}
	recs := make([]TraceRecord, n+1)
	// the tap's buffers live in C memory for the call (a struct passed to C may hold no Go pointers)
	nInfo := int(C.ISIM_DES_SPAN_INFO_WORDS)
	sizes := []int{8 * (maxTraces + 1), 8 * (maxTraces + 1), int(unsafe.Sizeof(DesSpan{})) * (capSpans + 1), 8 * nInfo, 8 * int(words)}
	bufs := make([]unsafe.Pointer, len(sizes))
	for i, b := range sizes {
		bufs[i] = C.calloc(1, C.size_t(b))
		defer C.free(bufs[i])
	}
	tap := (*C.isim_des_tap)(C.calloc(1, C.size_t(unsafe.Sizeof(C.isim_des_tap{}))))
	defer C.free(unsafe.Pointer(tap))
	tap.q_ppm = C.uint32_t(qPpm)
	tap.cls = C.ISIM_Q_ALL
	tap.max_traces = C.uint64_t(maxTraces)
	tap.cap_spans = C.uint64_t(capSpans)
	tap.d_ids = (*C.uint64_t)(bufs[0])
	tap.d_off = (*C.uint64_t)(bufs[1])
	tap.d_spans = (*C.isim_des_span)(bufs[2])
	tap.d_info = (*C.uint64_t)(bufs[3])
	tap.d_wait_table = (*C.uint64_t)(bufs[4])
	p := C.isim_des_params{mean_interarrival_ns: C.uint64_t(meanNs)}
	rc := C.isim_serve_des_spans(h.h, C.int(device), &p, nil, C.uint64_t(begin), C.uint64_t(n), &recs[0], nil, nil, tap)
	if err := lastErr(rc); err != nil {
		return nil, nil, nil, err
	}
	info := (*[1 << 3]uint64)(bufs[3])[:nInfo:nInfo]
	off := (*[1 << 30]uint64)(bufs[1])[: maxTraces+1 : maxTraces+1]
	written := int(info[C.ISIM_SPAN_WRITTEN])
	all := append([]DesSpan(nil), (*[1 << 24]DesSpan)(bufs[2])[:off[written]:off[written]]...)
	out := make([][]DesSpan, written)
	for i := range out {
		out[i] = all[off[i]:off[i+1]]
	}
	table := append([]uint64(nil), (*[1 << 30]uint64)(bufs[4])[:words:words]...)
	return recs[:n], out, table, nil
}

// DesWaitMerge adds src into dst (isim_des_wait_merge): sums, DwMaxWait by max.
func (h *Handler) DesWaitMerge(dst, src []uint64) error {
	return lastErr(C.isim_des_wait_merge(h.h, u64ptr(dst), u64ptr(src)))
}

// The DES critical-path table (DESIGN §22): (services + 1) rows of DcpRowWords
// words; row s the words below, the last row the header.  Tables merge by
// addition (DesCriticalPathMerge).
const (
	DcpInvocations    = C.ISIM_DCP_INVOCATIONS
	DcpSumDuration    = C.ISIM_DCP_SUM_DURATION
	DcpCritical       = C.ISIM_DCP_CRITICAL
	DcpWaitNs         = C.ISIM_DCP_WAIT_NS
	DcpSelfNs         = C.ISIM_DCP_SELF_NS
	DcpHopNs          = C.ISIM_DCP_HOP_NS
	DcpCritical500    = C.ISIM_DCP_CRITICAL_500
	DcpCriticalWaited = C.ISIM_DCP_CRITICAL_WAITED
	DcpRowWords       = C.ISIM_DCP_ROW_WORDS
	DcpHTraces        = C.ISIM_DCP_H_TRACES
	DcpHSpans         = C.ISIM_DCP_H_SPANS
	DcpHCritical      = C.ISIM_DCP_H_CRITICAL
	DcpHSumLatency    = C.ISIM_DCP_H_SUM_LATENCY
	DcpHRefused       = C.ISIM_DCP_H_REFUSED
)

// DesCriticalPath folds the traces ServeDesSpans returned on GPU `device`
// (isim_des_critical_path): it ORs SpanCritical into the status of the spans on
// each trace's critical path and returns the table and, per trace, the queue
// wait on its critical path (math.MaxUint64 for a refused trace).
func (h *Handler) DesCriticalPath(device int, traces [][]DesSpan) ([]uint64, []uint64, error) {
	var words C.uint64_t
	if err := lastErr(C.isim_des_critical_path_table_words(h.h, &words)); err != nil {
		return nil, nil, err
	}
	off := make([]uint64, len(traces)+1)
	for i, t := range traces {
		off[i+1] = off[i] + uint64(len(t))
	}
	all := make([]DesSpan, 0, off[len(traces)]+1)
	for _, t := range traces {
		all = append(all, t...)
	}
	table := make([]uint64, words)
	wait := make([]uint64, len(traces)+1)
	var sp *C.isim_des_span
	if len(all) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&all[0]))
	}
	rc := C.isim_des_critical_path(C.int(device), h.h, u64ptr(off), C.uint64_t(len(traces)), sp, u64ptr(table), u64ptr(wait))
	if err := lastErr(rc); err != nil {
		return nil, nil, err
	}
	for i, t := range traces {
		copy(t, all[off[i]:off[i+1]])
	}
	return table, wait[:len(traces)], nil
}

// DesCriticalPathMerge adds src into dst (isim_des_critical_path_merge).
func (h *Handler) DesCriticalPathMerge(dst, src []uint64) error {
	return lastErr(C.isim_des_critical_path_merge(h.h, u64ptr(dst), u64ptr(src)))
}

// The service timeline (DESIGN §23): per service (windows + 2) rows of
// SvtRowWords words (before t0, the windows, after them), then one header block.
// Tables merge by addition except SvtMaxWait (ServiceTimelineMerge).
const (
	SvtArrived  = C.ISIM_SVT_ARRIVED
	SvtStarted  = C.ISIM_SVT_STARTED
	SvtFinished = C.ISIM_SVT_FINISHED
	SvtSumWait  = C.ISIM_SVT_SUM_WAIT
	SvtMaxWait  = C.ISIM_SVT_MAX_WAIT
	SvtQueuedNs = C.ISIM_SVT_QUEUED_NS
	SvtBusyNs   = C.ISIM_SVT_BUSY_NS
	SvtRowWords = C.ISIM_SVT_ROW_WORDS
	SvtHFolded  = C.ISIM_SVT_H_FOLDED
	SvtHRefused = C.ISIM_SVT_H_REFUSED
)

func svtParams(t0Ns, windowNs uint64, nWindows uint32) C.isim_timeline_params {
	return C.isim_timeline_params{t0_ns: C.uint64_t(t0Ns), window_ns: C.uint64_t(windowNs), n_windows: C.uint32_t(nWindows)}
}

// ServiceHolds returns per service its worker hold in ns and its replicas
// (isim_des_service_holds): BusyNs / (window x replicas x workers) is the
// utilisation (DesWorkers: 1 each unless set).
func (h *Handler) ServiceHolds(nServices int) ([]uint64, []uint32, error) {
	hold, reps := make([]uint64, nServices+1), make([]uint32, nServices+1)
	rc := C.isim_des_service_holds(h.h, u64ptr(hold), (*C.uint32_t)(unsafe.Pointer(&reps[0])))
	if err := lastErr(rc); err != nil {
		return nil, nil, err
	}
	return hold[:nServices], reps[:nServices], nil
}

// ServiceTimeline folds spans (every span of a whole tapped batch, in any
// order) on GPU `device` into a new table (isim_service_timeline).
func (h *Handler) ServiceTimeline(device int, spans []DesSpan, t0Ns, windowNs uint64, nWindows uint32) ([]uint64, error) {
	p := svtParams(t0Ns, windowNs, nWindows)
	var words C.uint64_t
	if err := lastErr(C.isim_service_timeline_table_words(h.h, &p, &words)); err != nil {
		return nil, err
	}
	table := make([]uint64, words)
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	if err := lastErr(C.isim_service_timeline(C.int(device), h.h, &p, sp, C.uint64_t(len(spans)), u64ptr(table))); err != nil {
		return nil, err
	}
	return table, nil
}

// ServiceTimelineMerge adds src into dst, SvtMaxWait by max (isim_service_timeline_merge).
func (h *Handler) ServiceTimelineMerge(dst, src []uint64, t0Ns, windowNs uint64, nWindows uint32) error {
	p := svtParams(t0Ns, windowNs, nWindows)
	return lastErr(C.isim_service_timeline_merge(h.h, &p, u64ptr(dst), u64ptr(src)))
}

// Per-service percentiles (DESIGN §28): per service, measure (SvqWait,
// SvqService, SvqDuration) and class a cell of 1 + len(qPpm) words (the count,
// then the order statistics), then SvqHeaderWords words (SvqHFolded, SvqHRefused).
const (
	SvqWait        = C.ISIM_SVQ_WAIT
	SvqService     = C.ISIM_SVQ_SERVICE
	SvqDuration    = C.ISIM_SVQ_DURATION
	SvqMeasures    = C.ISIM_SVQ_MEASURES
	SvqClasses     = C.ISIM_SVQ_CLASSES
	SvqHFolded     = C.ISIM_SVQ_H_FOLDED
	SvqHRefused    = C.ISIM_SVQ_H_REFUSED
	SvqHeaderWords = C.ISIM_SVQ_HEADER_WORDS
)

// ServiceQuantiles selects, on GPU `device`, the exact percentiles qPpm of the
// queue wait, service time and duration of every service over spans (every span
// of a whole tapped batch, in any order) into a new table (isim_service_quantiles).
func (h *Handler) ServiceQuantiles(device int, spans []DesSpan, qPpm []uint32) ([]uint64, error) {
	var words C.uint64_t
	if err := lastErr(C.isim_service_quantiles_table_words(h.h, C.uint32_t(len(qPpm)), &words)); err != nil {
		return nil, err
	}
	table := make([]uint64, words)
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	q := u32ptr(qPpm)
	if err := lastErr(C.isim_service_quantiles(C.int(device), h.h, q, C.uint32_t(len(qPpm)), sp, C.uint64_t(len(spans)), u64ptr(table))); err != nil {
		return nil, err
	}
	return table, nil
}

// ServiceQuantilesHost is ServiceQuantiles on the CPU (isim_service_quantiles_host).
func (h *Handler) ServiceQuantilesHost(spans []DesSpan, qPpm []uint32) ([]uint64, error) {
	var words C.uint64_t
	if err := lastErr(C.isim_service_quantiles_table_words(h.h, C.uint32_t(len(qPpm)), &words)); err != nil {
		return nil, err
	}
	table := make([]uint64, words)
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	q := u32ptr(qPpm)
	if err := lastErr(C.isim_service_quantiles_host(h.h, q, C.uint32_t(len(qPpm)), sp, C.uint64_t(len(spans)), u64ptr(table))); err != nil {
		return nil, err
	}
	return table, nil
}

// Per-service latency sketch (DESIGN §30): per service and measure (SvqWait,
// SvqService, SvqDuration) a latency-sketch table by code and bin, then
// SvqHeaderWords words.  Every word is a count: tables of many batches and
// GPUs merge by addition.
const (
	SvsMaxWords = C.ISIM_SVS_MAX_WORDS
	SvsShort    = C.ISIM_SVS_SHORT
)

// NewServiceSketch is a zeroed table of subBits (isim_service_sketch_table_words).
func (h *Handler) NewServiceSketch(subBits uint32) ([]uint64, error) {
	var words C.uint64_t
	if err := lastErr(C.isim_service_sketch_table_words(h.h, C.uint32_t(subBits), &words)); err != nil {
		return nil, err
	}
	return make([]uint64, words), nil
}

// ServiceSketch adds, on GPU `device`, spans (every span of a whole tapped
// batch, in any order) into table, a NewServiceSketch of the same subBits
// (isim_service_sketch).
func (h *Handler) ServiceSketch(device int, subBits uint32, spans []DesSpan, table []uint64) error {
	if err := h.serviceSketchTable(subBits, table); err != nil {
		return err
	}
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	return lastErr(C.isim_service_sketch(C.int(device), h.h, C.uint32_t(subBits), sp, C.uint64_t(len(spans)), u64ptr(table)))
}

// ServiceSketchHost is ServiceSketch on the CPU (isim_service_sketch_host).
func (h *Handler) ServiceSketchHost(subBits uint32, spans []DesSpan, table []uint64) error {
	if err := h.serviceSketchTable(subBits, table); err != nil {
		return err
	}
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	return lastErr(C.isim_service_sketch_host(h.h, C.uint32_t(subBits), sp, C.uint64_t(len(spans)), u64ptr(table)))
}

// ServiceSketchMerge adds every word of src to dst, the header included
// (isim_service_sketch_merge).
func (h *Handler) ServiceSketchMerge(subBits uint32, dst, src []uint64) error {
	if err := h.serviceSketchTable(subBits, dst); err != nil {
		return err
	}
	if err := h.serviceSketchTable(subBits, src); err != nil {
		return err
	}
	return lastErr(C.isim_service_sketch_merge(h.h, C.uint32_t(subBits), u64ptr(dst), u64ptr(src)))
}

// ServiceSketchQuantiles gives, per service and measure, SketchQuantiles' words
// of that block: [services][SvqMeasures][3 classes][1 + 2 * len(qPpm)], per class
// the count, then lo and hi per quantile (isim_service_sketch_quantiles).
func (h *Handler) ServiceSketchQuantiles(subBits uint32, table []uint64, qPpm []uint32) ([]uint64, error) {
	if err := h.serviceSketchTable(subBits, table); err != nil {
		return nil, err
	}
	blocks := (uint64(len(table)) - SvqHeaderWords) / (2 * ((65 - uint64(subBits)) << subBits))
	out := make([]uint64, blocks*3*(1+2*uint64(len(qPpm)))+1)
	if err := lastErr(C.isim_service_sketch_quantiles(h.h, C.uint32_t(subBits), u64ptr(table), u32ptr(qPpm), C.uint32_t(len(qPpm)), u64ptr(out))); err != nil {
		return nil, err
	}
	return out[:len(out)-1], nil
}

// serviceSketchTable refuses a table that is not of this handler and subBits.
func (h *Handler) serviceSketchTable(subBits uint32, table []uint64) error {
	var words C.uint64_t
	if err := lastErr(C.isim_service_sketch_table_words(h.h, C.uint32_t(subBits), &words)); err != nil {
		return err
	}
	if uint64(len(table)) != uint64(words) {
		return fmt.Errorf("isim: a service sketch of %d words, want %d", len(table), uint64(words))
	}
	return nil
}

// Per-service percentiles over time (DESIGN §29): per service, timeline row
// (0 before t0Ns, 1 .. nWindows the windows, nWindows + 1 after; the row of a
// span's finish), measure and class a cell of 1 + len(qPpm) words as in
// ServiceQuantiles, then SvqHeaderWords words.
const (
	SwqMaxCells = C.ISIM_SWQ_MAX_CELLS
	SwqWave     = C.ISIM_SWQ_WAVE
)

// ServiceWindowQuantilesWorkspaceBytes is the workspace the device call
// (C.isim_service_window_quantiles_device) needs for capSpans spans
// (isim_service_window_quantiles_workspace_bytes).
func (h *Handler) ServiceWindowQuantilesWorkspaceBytes(capSpans uint64, nQ int, t0Ns, windowNs uint64, nWindows uint32) (uint64, error) {
	p := svtParams(t0Ns, windowNs, nWindows)
	var bytes C.uint64_t
	if err := lastErr(C.isim_service_window_quantiles_workspace_bytes(h.h, &p, C.uint64_t(capSpans), C.uint32_t(nQ), &bytes)); err != nil {
		return 0, err
	}
	return uint64(bytes), nil
}

// ServiceWindowQuantiles selects, on GPU `device`, the exact percentiles qPpm
// of the queue wait, service time and duration of every service and timeline
// row over spans (every span of a whole tapped batch, in any order) into a new
// table (isim_service_window_quantiles).
func (h *Handler) ServiceWindowQuantiles(device int, spans []DesSpan, qPpm []uint32, t0Ns, windowNs uint64, nWindows uint32) ([]uint64, error) {
	p := svtParams(t0Ns, windowNs, nWindows)
	var words C.uint64_t
	if err := lastErr(C.isim_service_window_quantiles_table_words(h.h, &p, C.uint32_t(len(qPpm)), &words)); err != nil {
		return nil, err
	}
	table := make([]uint64, words)
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	q := u32ptr(qPpm)
	if err := lastErr(C.isim_service_window_quantiles(C.int(device), h.h, &p, q, C.uint32_t(len(qPpm)), sp, C.uint64_t(len(spans)), u64ptr(table))); err != nil {
		return nil, err
	}
	return table, nil
}

// ServiceWindowQuantilesHost is ServiceWindowQuantiles on the CPU
// (isim_service_window_quantiles_host).
func (h *Handler) ServiceWindowQuantilesHost(spans []DesSpan, qPpm []uint32, t0Ns, windowNs uint64, nWindows uint32) ([]uint64, error) {
	p := svtParams(t0Ns, windowNs, nWindows)
	var words C.uint64_t
	if err := lastErr(C.isim_service_window_quantiles_table_words(h.h, &p, C.uint32_t(len(qPpm)), &words)); err != nil {
		return nil, err
	}
	table := make([]uint64, words)
	var sp *C.isim_des_span
	if len(spans) > 0 {
		sp = (*C.isim_des_span)(unsafe.Pointer(&spans[0]))
	}
	q := u32ptr(qPpm)
	if err := lastErr(C.isim_service_window_quantiles_host(h.h, &p, q, C.uint32_t(len(qPpm)), sp, C.uint64_t(len(spans)), u64ptr(table))); err != nil {
		return nil, err
	}
	return table, nil
}

// SelectTraces returns the ids begin + i of the records with a latency of at
// least minLatencyNs in class cls (C.ISIM_Q_ALL / ISIM_Q_200 / ISIM_Q_500), in
// ascending i, at most maxIDs of them, and the number of matching records
// (isim_select_traces, on GPU `device`).
func SelectTraces(device int, recs []TraceRecord, begin, minLatencyNs uint64, cls uint32, maxIDs int) ([]uint64, uint64, error) {
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	if maxIDs > len(recs) {
		maxIDs = len(recs)
	}
	ids := make([]uint64, maxIDs)
	info := make([]uint64, 2)
	rc := C.isim_select_traces(C.int(device), rp, C.uint64_t(len(recs)), C.uint64_t(begin), C.uint64_t(minLatencyNs),
		C.uint32_t(cls), C.uint64_t(maxIDs), u64ptr(ids), u64ptr(info))
	if err := lastErr(rc); err != nil {
		return nil, 0, err
	}
	return ids[:info[1]], info[0], nil
}

// TimelineRow is one row of a timeline table: the requests that arrived in
// the window and, of those that completed in it, by code (0: 200, 1: 500),
// their count, latency sum, latency maximum and Prometheus histogram.
type TimelineRow struct {
	Arrived uint64
	Done    [2]uint64
	SumLat  [2]uint64
	MaxLat  [2]uint64
	Prom    [2][]uint64
}

// Timeline bins arrivals and records into nWindows windows of windowNs from
// t0Ns on GPU `device` (isim_timeline).  Rows: "before" t0Ns, the windows,
// "after" the last window.
func Timeline(device int, arrivals []uint64, recs []TraceRecord, t0Ns, windowNs uint64, nWindows uint32) ([]TimelineRow, error) {
	if len(arrivals) != len(recs) {
		return nil, errors.New("arrivals and records differ in length")
	}
	p := C.isim_timeline_params{t0_ns: C.uint64_t(t0Ns), window_ns: C.uint64_t(windowNs), n_windows: C.uint32_t(nWindows)}
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	if nWindows < 1 || nWindows > C.ISIM_TL_MAX_WINDOWS {
		// libisim's EINVAL and message; the output is never written
		return nil, lastErr(C.isim_timeline(C.int(device), u64ptr(arrivals), rp, C.uint64_t(len(recs)), &p, nil))
	}
	const w = C.ISIM_TL_ROW_WORDS
	out := make([]uint64, (int(nWindows)+2)*w)
	rc := C.isim_timeline(C.int(device), u64ptr(arrivals), rp, C.uint64_t(len(recs)), &p, u64ptr(out))
	if rc != C.ISIM_OK {
		return nil, lastErr(rc)
	}
	rows := make([]TimelineRow, int(nWindows)+2)
	for i := range rows {
		r := out[i*w : (i+1)*w]
		rows[i].Arrived = r[C.ISIM_TL_ARRIVED]
		for c := 0; c < 2; c++ {
			rows[i].Done[c] = r[C.ISIM_TL_DONE+c]
			rows[i].SumLat[c] = r[C.ISIM_TL_SUM_LAT+c]
			rows[i].MaxLat[c] = r[C.ISIM_TL_MAX_LAT+c]
			rows[i].Prom[c] = r[C.ISIM_TL_PROM+c*C.ISIM_N_PROM : C.ISIM_TL_PROM+(c+1)*C.ISIM_N_PROM]
		}
	}
	return rows, nil
}

// TimelineQuantiles computes, for every row of the Timeline table ("before"
// t0Ns, the nWindows windows of windowNs, "after" the last), the exact
// latency percentiles of the records that complete in it on GPU `device`
// (isim_timeline_quantiles): per row the classes of LatencyQuantiles
// (C.ISIM_Q_ALL / ISIM_Q_200 / ISIM_Q_500).  qPpm as in LatencyQuantiles.
func TimelineQuantiles(device int, arrivals []uint64, recs []TraceRecord, t0Ns, windowNs uint64, nWindows uint32, qPpm []uint32) ([][3]Quantiles, error) {
	if len(arrivals) != len(recs) {
		return nil, errors.New("arrivals and records differ in length")
	}
	p := C.isim_timeline_params{t0_ns: C.uint64_t(t0Ns), window_ns: C.uint64_t(windowNs), n_windows: C.uint32_t(nWindows)}
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0]
	}
	var qp *C.uint32_t
	if len(qPpm) > 0 {
		qp = (*C.uint32_t)(unsafe.Pointer(&qPpm[0]))
	}
	nq := len(qPpm)
	if nWindows < 1 || nWindows > C.ISIM_TL_MAX_WINDOWS || nq < 1 || nq > C.ISIM_MAX_QUANTILES {
		// libisim's EINVAL and message; the output is never written
		return nil, lastErr(C.isim_timeline_quantiles(C.int(device), u64ptr(arrivals), rp, C.uint64_t(len(recs)), &p, qp, C.uint32_t(nq), nil))
	}
	w := 3 * (1 + nq) // ISIM_Q_OUT_WORDS per row: ISIM_TLQ_OUT_WORDS (cgo sees no function-like macros)
	out := make([]uint64, (int(nWindows)+2)*w)
	rc := C.isim_timeline_quantiles(C.int(device), u64ptr(arrivals), rp, C.uint64_t(len(recs)), &p, qp, C.uint32_t(nq), u64ptr(out))
	if rc != C.ISIM_OK {
		return nil, lastErr(rc)
	}
	rows := make([][3]Quantiles, int(nWindows)+2)
	for i := range rows {
		for c := 0; c < 3; c++ {
			r := out[i*w+c*(1+nq) : i*w+(c+1)*(1+nq)]
			rows[i][c] = Quantiles{Count: r[0], Values: r[1:]}
		}
	}
	return rows, nil
}

type Multi struct{ m *C.isim_multi }

// u64ptr passes an empty slice as NULL (libisim then reports EINVAL) instead
// of panicking on &s[0].
func u32ptr(s []uint32) *C.uint32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&s[0]))
}

func u64ptr(s []uint64) *C.uint64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&s[0]))
}

// NewMultiNode drives every listed device from this process (ncclCommInitAll).
func NewMultiNode(devices []int32) (*Multi, error) {
	var m *C.isim_multi
	if len(devices) == 0 {
		return nil, lastErr(C.isim_multi_init_all(nil, 0, &m)) // libisim's EINVAL and message
	}
	rc := C.isim_multi_init_all((*C.int)(unsafe.Pointer(&devices[0])), C.int(len(devices)), &m)
	return &Multi{m}, lastErr(rc)
}

// MultiPrecheck makes the local checks of NewMultiRank (RCCL loads, the
// device can be selected) before the collective creation, so the ranks can
// agree on them out of band first.
func MultiPrecheck(device int) error { return lastErr(C.isim_multi_precheck(C.int(device))) }

// MultiID is created on rank 0 and shipped to the other ranks (e.g. over gRPC).
func MultiID() ([128]byte, error) {
	var id C.isim_multi_id
	rc := C.isim_multi_get_id(&id)
	return *(*[128]byte)(unsafe.Pointer(&id)), lastErr(rc)
}

func NewMultiRank(id [128]byte, nRanks, rank, device int) (*Multi, error) {
	var m *C.isim_multi
	rc := C.isim_multi_init_rank((*C.isim_multi_id)(unsafe.Pointer(&id)), C.int(nRanks), C.int(rank),
		C.int(device), &m)
	return &Multi{m}, lastErr(rc)
}

func (m *Multi) Close() { C.isim_multi_free(m.m) }

// ServeSharded walks this process's shards of [begin, begin + nRanks*perRank)
// and returns the node-wide merged stats (identical on every rank).
func (h *Handler) ServeSharded(m *Multi, begin, perRank uint64, recs []TraceRecord) ([]uint64, error) {
	var info C.isim_handler_info
	if rc := C.isim_handler_info_get(h.h, &info); rc != C.ISIM_OK {
		return nil, lastErr(rc)
	}
	stats := make([]uint64, int(info.stats_words))
	var rp *TraceRecord
	if len(recs) > 0 {
		rp = &recs[0] // n_local * perRank records
	}
	rc := C.isim_serve_multi(h.h, m.m, C.uint64_t(begin), C.uint64_t(perRank), rp,
		u64ptr(stats))
	return stats, lastErr(rc)
}

// Abort makes the peers' pending or next collectives fail (isim_multi_abort)
// instead of waiting for a rank that failed before a collective.
func (m *Multi) Abort() error { return lastErr(C.isim_multi_abort(m.m)) }

// K8sOptions are the arguments of kubernetes.ServiceGraphToKubernetesManifests
// (isotope/convert/pkg/kubernetes/kubernetes.go:56-63) plus the two EXT
// determinism knobs (creationTimestamp, RBAC rule names).
type K8sOptions struct {
	ServiceNodeSelector              map[string]string
	ServiceImage                     string
	ServiceMaxIdleConnectionsPerHost int
	ClientNodeSelector               map[string]string
	ClientImage                      string
	EnvironmentName                  string // "NONE" or "ISTIO"
	CreationTimestampUnix            int64
	RbacSeed                         uint64
}

func cStrings(m map[string]string) (**C.char, C.int32_t, func()) {
	if len(m) == 0 {
		return nil, 0, func() {}
	}
	arr := C.malloc(C.size_t(2*len(m)) * C.size_t(unsafe.Sizeof(uintptr(0))))
	ptrs := (*[1 << 28]*C.char)(arr)[: 2*len(m) : 2*len(m)]
	i := 0
	for k, v := range m {
		ptrs[i], ptrs[i+1] = C.CString(k), C.CString(v)
		i += 2
	}
	return (**C.char)(arr), C.int32_t(len(m)), func() {
		for _, p := range ptrs {
			C.free(unsafe.Pointer(p))
		}
		C.free(arr)
	}
}

// KubernetesManifests mirrors kubernetes.ServiceGraphToKubernetesManifests.
func (g *Graph) KubernetesManifests(o K8sOptions) ([]byte, error) {
	var p C.isim_k8s_params
	si, ci, env := C.CString(o.ServiceImage), C.CString(o.ClientImage), C.CString(o.EnvironmentName)
	defer C.free(unsafe.Pointer(si))
	defer C.free(unsafe.Pointer(ci))
	defer C.free(unsafe.Pointer(env))
	ss, sn, sfree := cStrings(o.ServiceNodeSelector)
	defer sfree()
	cs, cn, cfree := cStrings(o.ClientNodeSelector)
	defer cfree()
	p.service_image, p.client_image, p.environment_name = si, ci, env
	p.service_node_selector, p.n_service_node_selector = ss, sn
	p.client_node_selector, p.n_client_node_selector = cs, cn
	p.service_max_idle_connections_per_host = C.int32_t(o.ServiceMaxIdleConnectionsPerHost)
	p.creation_timestamp_s = C.int64_t(o.CreationTimestampUnix)
	p.rbac_seed = C.uint64_t(o.RbacSeed)
	s, err := g.text(func(a *C.isim_graph, b *C.char, c C.size_t, d *C.size_t) C.int {
		return C.isim_graph_to_k8s_manifests(a, &p, b, c, d)
	})
	return []byte(s), err
}

// MarshalYAML returns yaml.Marshal(graph) as sigs.k8s.io/yaml renders it.
func (g *Graph) MarshalYAML() ([]byte, error) {
	s, err := g.text(func(a *C.isim_graph, b *C.char, c C.size_t, d *C.size_t) C.int {
		return C.isim_graph_marshal_yaml(a, b, c, d)
	})
	return []byte(s), err
}
