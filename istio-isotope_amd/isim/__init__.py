"""isim — MI355X-native simulator of isotope service-graph request traces.

Host-side mirror of isotope's graph and handler API over libisim.so
(include/isim.h).  See DESIGN.md.
"""
from .graph import (ConcurrentCommand, GraphError, RequestCommand, Service, ServiceGraph,  # noqa: F401
                    SleepCommand, duration_parse, percentage_from_string, size_from_string)
from .native import ECOMM, MODE_A, MODE_B, IsimError  # noqa: F401
from .sim import REC_DTYPE, Handler, SimParams, decode_stats, handler_from_service_graph_yaml  # noqa: F401
from .yamljson import yaml_to_json  # noqa: F401
from . import prometheus  # noqa: F401
from .des import DesHandler  # noqa: F401
from .load_profile import (LoadProfile, profile_arrivals, profile_arrivals_device,  # noqa: F401
                           profile_arrivals_workspace_bytes)
from .closed_loop import (ClosedLoop, ClosedLoopRun, closed_loop_workspace_bytes,  # noqa: F401
                          decode_closed_loop_info)
from .quantiles import (DEFAULT_Q, latency_quantiles, latency_quantiles_device, quantile_rank,  # noqa: F401
                        quantiles_out_words, quantiles_workspace_bytes)
from .timeline import (decode_timeline, des_arrivals, des_arrivals_device, des_arrivals_workspace_bytes,  # noqa: F401
                       timeline, timeline_device, timeline_merge, timeline_out_words, timeline_table)
from .timeline_quantiles import (decode_timeline_quantiles, timeline_quantiles, timeline_quantiles_device,  # noqa: F401
                                 timeline_quantiles_out_words, timeline_quantiles_table,
                                 timeline_quantiles_workspace_bytes)
from .sketch import (decode_timeline_sketch, latency_sketch, latency_sketch_device, sketch_bins,  # noqa: F401
                     sketch_bounds, sketch_bucket, sketch_merge, sketch_quantiles, sketch_words, timeline_sketch,
                     timeline_sketch_device, timeline_sketch_out_words, timeline_sketch_table)
from .des_spans import (DES_SPAN_DTYPE, DesCriticalPath, DesTrace, DesWaitTable,  # noqa: F401
                        des_critical_path_device, des_critical_path_host)
from .spans import (SPAN_DTYPE, CriticalPath, Trace, TraceSpans, select_traces, select_traces_device,  # noqa: F401
                    select_traces_host, select_workspace_bytes)
from .service_timeline import (ServiceTimeline, service_holds, service_timeline, service_timeline_device,  # noqa: F401
                               service_timeline_host, service_timeline_table_words,
                               service_timeline_workspace_bytes)
from .service_quantiles import (MEASURE_NAMES, ServiceQuantiles, decode_service_quantiles,  # noqa: F401
                                service_quantiles, service_quantiles_device, service_quantiles_host,
                                service_quantiles_table_words, service_quantiles_workspace_bytes)
from .service_sketch import (ServiceSketch, service_sketch, service_sketch_device, service_sketch_host,  # noqa: F401
                             service_sketch_merge, service_sketch_quantiles, service_sketch_table_words,
                             service_sketch_workspace_bytes)
from .service_window_quantiles import (ServiceWindowQuantiles, decode_service_window_quantiles,  # noqa: F401
                                       service_window_quantiles, service_window_quantiles_device,
                                       service_window_quantiles_host, service_window_quantiles_table_words,
                                       service_window_quantiles_workspace_bytes)
