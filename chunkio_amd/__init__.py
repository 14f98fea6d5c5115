"""chunkio_amd -- MI355X-native replacement of fluent/chunkio's CRC-32
content-checksum path (and its SHA-1 content hash).

Layers:
  include/crc32/crc32.h, include/chunkio_amd/*.h   C ABI (the drop-in boundary)
  chunkio_amd/csrc/*.hip, *.c                      HIP kernels for gfx950 + host C
  chunkio_amd/crc32.py                             Python mirror of the CRC and SHA-1 API
                                                   (Sha1 / sha1_hash: chunkio's cio_sha1 on
                                                   OpenSSL-layout SHA_CTX bytes)
  chunkio_amd/chunkfile.py                         binding of the C chunk layer
                                                   (cioa_chunk.h: write/sync/verify/tx/scan,
                                                   up_batch) and of the device-side write
                                                   path (cio_write_dev.h: DevWriter,
                                                   init / write / seal_batch_dev;
                                                   cio_write_dev_move.h:
                                                   write_metadata / write_at_batch_dev;
                                                   cio_write_dev_records.h:
                                                   write_records_batch_dev;
                                                   cio_write_dev_ungrouped.h:
                                                   write_records_ungrouped_batch_dev;
                                                   cio_write_dev_grow.h:
                                                   grow_batch_dev / grow_records_batch_dev;
                                                   cio_write_dev_rotate.h:
                                                   rotate_batch_dev / rotate_records_batch_dev;
                                                   cio_write_dev_pool.h:
                                                   pool_state, release_batch_dev,
                                                   rotate_pool_batch_dev /
                                                   rotate_pool_records_batch_dev;
                                                   cio_write_dev_pool_set.h:
                                                   pool_set_state, pool_set_class,
                                                   release_set_batch_dev, grow_set_batch_dev /
                                                   grow_set_records_batch_dev;
                                                   cio_write_dev_coalesce.h:
                                                   coalesce_set_dev;
                                                   cio_route_dev.h:
                                                   route_dir, route_build_dev,
                                                   route_records_batch_dev;
                                                   cio_persist_dev.h:
                                                   alloc_set_batch_dev, load_paths_dev,
                                                   store_paths_dev, persist_round_max,
                                                   persist_rounds, persist_trim;
                                                   cio_write_dev_tx.h:
                                                   tx_state, tx_begin / tx_rollback /
                                                   tx_commit / tx_cond_records_batch_dev)
                                                   and read path (cio_read_dev.h:
                                                   read / read_packed / meta_cmp_batch_dev)
"""
from ._lib import LIB_PATH, CioGpuError, lib  # noqa: F401
from .crc32 import (  # noqa: F401
    CRC_INIT, DEVPLAN_E_BATCH_TOO_LARGE, DEVPLAN_E_BOUNDS, DEVPLAN_E_CHUNK_TOO_LARGE, Crc32DevPlan, Crc32Plan, Crc32Ring, crc32, crc32_batch_cpu_packed, crc32_batch_dev, crc32_batch_host, crc32_batch_host_packed,
    crc32_combine, crc32_split_host, host_threads,
    crc32_shift, crc_finalize, crc_init, crc_update, device_count, fill_synthetic, host_register,
    host_unregister, pipe_last_timing, plan_cache_stats, split_rates, route, Sha1, sha1_hash, sha1_to_hex, sha1_batch_dev, sha1_batch_dev_async, sha1_final_batch_dev,
    sha1_states_init, sha1_states_view, sha1_update_batch_dev,
)

from .chunkfile import (  # noqa: F401,E402
    CIOA_GROW_ZERO, CIOA_TX_RECOMPUTE, CIOA_TX_ZERO, CIOA_READ_CONTENT, CIOA_READ_IMAGE, CIOA_READ_META, CIOA_READ_NUL, CIOA_SEAL_RECOMPUTE, CIOA_WRITER_MOVE,
    DevWriter, grow_batch_dev, grow_records_batch_dev, init_batch_dev, meta_cmp_batch_dev, read_batch_dev, read_packed_batch_dev,
    rotate_batch_dev, rotate_records_batch_dev, seal_batch_dev,
    CIOA_RELEASE_COMPACT, CIOA_RELEASE_ZERO, pool_state, release_batch_dev, rotate_pool_batch_dev,
    rotate_pool_records_batch_dev,
    CIOA_POOL_SET_MAX, grow_set_batch_dev, grow_set_records_batch_dev, pool_set_class, pool_set_state,
    release_set_batch_dev,
    COALESCE_DRY, coalesce_set_dev,
    route_build_dev, route_dir, route_records_batch_dev,
    CIOA_ALLOC_ZERO, CIOA_LOAD_ZERO, CIOA_STORE_SYNC, CIOA_STORE_TRIM, alloc_set_batch_dev, load_paths_dev,
    persist_round_max, persist_rounds, persist_trim, store_paths_dev,
    tx_begin_batch_dev, tx_commit_batch_dev, tx_cond_records_batch_dev, tx_rollback_batch_dev, tx_state,
    verify_batch_dev, write_at_batch_dev, write_batch_dev, write_metadata_batch_dev, write_records_batch_dev,
    write_records_ungrouped_batch_dev,
)

__version__ = "0.5.0"
