"""Device-planned CRC-32 and device verify-on-load: the argument checks of the
new C entry points run before any device call, so they hold without a GPU."""
import ctypes

import chunkio_amd
from chunkio_amd import chunkfile as cf


def test_devplan_create_rejects_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    h = ctypes.c_void_p()
    assert lib.cio_crc32_devplan_create(None, 16) == -1
    assert b"null argument" in lib.cio_gpu_last_error()
    for bad in (0, (1 << 32) - 1, 1 << 32):
        assert lib.cio_crc32_devplan_create(ctypes.byref(h), bad) == -1, bad
        assert b"max_chunks" in lib.cio_gpu_last_error()
        assert not h.value
    lib.cio_crc32_devplan_destroy(None)       # a no-op


def test_devplan_exec_rejects_null_plan_without_a_gpu():
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    assert lib.cio_crc32_devplan_exec(None, buf, 64, buf, buf, 1, None, buf, None, None) == -1
    assert b"null plan" in lib.cio_gpu_last_error()
    assert lib.cio_crc32_devplan_exec(None, buf, 64, buf, buf, 0, None, buf, None, None) == -1
    assert b"null plan" in lib.cio_gpu_last_error()
    assert lib.cio_crc32_devplan_workgroups(None) == 0


def test_devplan_entry_points_reject_null_buffers_without_a_gpu():
    """Null buffers are refused before the plan is looked at (`plan` here is
    just a non-null address), and an empty batch is a no-op."""
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    plan = ctypes.create_string_buffer(256)
    for k in (1, 3, 4, 7):                        # dev_base, dev_offs, dev_lens, dev_out
        a = [plan, buf, 64, buf, buf, 1, None, buf, None, None]
        a[k] = None
        assert lib.cio_crc32_devplan_exec(*a) == -1, k
        assert b"null pointer" in lib.cio_gpu_last_error()
    assert lib.cio_crc32_devplan_exec(plan, None, 0, None, None, 0, None, None, None, None) == 0
    for k in (1, 3, 4, 7, 8, 9):                  # dev_base, img_offs, img_sizes, status, error, crc_raw
        a = [plan, buf, 64, buf, buf, 1, cf.CIO_CHECKSUM, buf, buf, buf, None, None, None]
        a[k] = None
        assert lib.cio_file_verify_batch_dev(*a) == -1, k
        assert b"null pointer" in lib.cio_gpu_last_error()
    assert lib.cio_file_verify_batch_dev(plan, None, 0, None, None, 0, 0, None, None, None, None, None, None) == 0


def test_verify_batch_dev_rejects_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    args = (buf, 64, buf, buf, 1)
    outs = (buf, buf, buf, buf, buf, None)
    # a device image cannot be written back or deleted
    for flags in (cf.CIOA_VERIFY_WRITEBACK, cf.CIOA_VERIFY_DELETE_IRRECOVERABLE,
                  cf.CIO_CHECKSUM | cf.CIOA_VERIFY_WRITEBACK, cf.CIO_CHECKSUM | cf.CIOA_VERIFY_DELETE_IRRECOVERABLE):
        assert lib.cio_file_verify_batch_dev(buf, *args, flags, *outs) == -1, flags
        assert b"only CIOA_VERIFY_CHECKSUM" in lib.cio_gpu_last_error()
    for flags in (0, cf.CIO_CHECKSUM):
        assert lib.cio_file_verify_batch_dev(None, *args, flags, *outs) == -1
        assert b"null plan" in lib.cio_gpu_last_error()


def test_python_binding_exports():
    assert chunkio_amd.Crc32DevPlan.exec and chunkio_amd.Crc32DevPlan.status
    assert chunkio_amd.verify_batch_dev is cf.verify_batch_dev
