"""The random walk over the device API on chunk images (lifecycle_walk.py) on
the models alone: the composed models against the ledger, which knows only
which records were accepted, and at the end every chunk against the host chunk
layer's loader (Context.scan, which test_ref_chunks.py pins to the reference's)
and against zlib.  The walk and the models are thereby tested without a GPU;
test_gpu_lifecycle_walk.py runs the same walks against the kernels."""
import os

import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import lifecycle_walk as lw


@pytest.fixture
def host_route():
    cio.route(reset=True, cpu_max=1 << 62, threads=1)
    yield
    cio.route(reset=True)


@pytest.mark.parametrize("seed", lw.SEEDS)
@pytest.mark.parametrize("profile", sorted(lw.PROFILES))
def test_walk_on_the_models(profile, seed, tmp_path, host_route):
    """walk() compares list + live with the ledger every 10 ops and at the end
    and asserts the coverage floors; its last op seals every image.  Then each
    finished or sealed chunk: its CRC field is zlib's over [22, 24 + meta +
    content), the host chunk layer loads it, and what it loads is the ledger's
    metadata and content."""
    s, ledger, _ = lw.walk(profile, seed)
    chunks = lw.sealed_chunks(s, ledger)
    assert len(chunks) == s.count[0] + s.n - len(s.bad)
    d = tmp_path / "root" / "walk"
    d.mkdir(parents=True)
    for name, image, meta, content in chunks:
        assert lw.crc_field_ok(image), (profile, seed, name, "CRC field")
        assert image[24:24 + len(meta)] == meta and image[24 + len(meta):] == content, (profile, seed, name)
        with open(d / name, "wb") as f:
            f.write(image)
    with cf.Context(str(tmp_path / "root"), cf.CIO_CHECKSUM, max_chunks_up=len(chunks) + 8) as ctx:
        _, loaded = ctx.scan("walk")
        got = {c.name: (bytes(c.map[24:24 + c.meta_len()]), c.content()) for c in loaded}
    want = {name: (meta, content) for name, _, meta, content in chunks}
    assert sorted(got) == sorted(want), (profile, seed, "refused by the loader", sorted(set(want) - set(got))[:8])
    assert got == want, (profile, seed, [n for n in want if got[n] != want[n]][:8])
