"""spiral_amd -- MI355X-native Spiral server-answer path.

The compute lives in libspiral_gpu.so (hand-written HIP for gfx950 behind the C ABI of
include/spiral_gpu.h).  This package is the thin host-side mirror of the reference's function
interface for that path (names and argument meaning of src/spiral.cpp / src/poly.cpp / src/core.cpp),
used by the parity tests and the benchmark.  numpy uint64 arrays carry the reference layouts.
"""
from ._lib import KV_ENTRY_DTYPE, KvReconcile, KvScan, KvScanOverflow, kv_reconcile  # noqa: F401
from ._lib import KvLayout, KvStats, PackShape, Params, RecordLayout, Shape, SpiralGpuError, build, db_items_bytes, kv_hash, kv_layout, lib, pack_kv_layout, record_layout  # noqa: F401
from ._lib import FINGERPRINT_MODULUS, fingerprint_add, fingerprint_host, fingerprint_of_polys  # noqa: F401
from .client import Client, ResponseNoise, client_noise_table  # noqa: F401
from .keys import KeyStore, bind_keys  # noqa: F401
from .ops import *  # noqa: F401,F403
from .pack import PackServer, fastMultiplyQueriesByDatabaseDim1, fastMultiplyQueryByDatabaseDim1, get_pack_shape, pack  # noqa: F401
from .pack import answer_batch_instances as pack_answer_batch_instances, answer_instances as pack_answer_instances  # noqa: F401
from .server import Server, answer_batch_instances, first_dim_batch, run_query_batch, run_query_batch_instances, time_sweep_batch  # noqa: F401
from .server import read_response_wire_batch, set_query_batch  # noqa: F401
from .server import fold_local_batch, fold_root_batch, run_expand_pack_batch, run_pre_sweep_batch, run_unpack_convert_sweep_batch  # noqa: F401
from .server import run_column_batch  # noqa: F401
