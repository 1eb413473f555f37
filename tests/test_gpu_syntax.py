"""GPU: the device parse (parse.hip through mp2vg_batch_upload_es) on the directed slice-syntax
streams of tests/golden/syntax (written by tests/directed_syntax.py, an independent writer; pinned
by the compiled reference's frame MD5s).  For every stream the records the kernels leave in HBM
equal the host emitter's byte for byte, and the frames decoded from the device-parsed and from the
host-parsed records have the reference's MD5s; the out-of-contract streams are rejected with the
host emitter's status and reason.  Reads only the committed fixture."""
import json
import os

import pytest

from conftest import GOLDEN
from helpers import yuv_md5
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu

SYNTAX = os.path.join(GOLDEN, "syntax")
with open(os.path.join(SYNTAX, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
POSITIVE = [e for e in MANIFEST if e["md5"] is not None]
NEGATIVE = [e for e in MANIFEST if e["md5"] is None]


@pytest.fixture(scope="module", autouse=True)
def _torch_runtime_first():
    """as in test_gpu_device_parse.py: torch's HIP runtime opens the device before the library's"""
    import torch
    torch.zeros(1, device="cuda")


def _read(e):
    with open(os.path.join(SYNTAX, e["file"]), "rb") as f:
        return f.read()


def _geom(e):
    return e["width"], e["height"], e["chroma_format"]


def _detail(msg):
    return msg.split("(", 1)[1]


@pytest.mark.parametrize("entry", POSITIVE, ids=[e["name"] for e in POSITIVE])
def test_device_records_are_the_hosts_and_frames_are_the_references(entry):
    es = _read(entry)
    parsed, scan = R.Parsed(es, *_geom(entry)), R.Scan(es, *_geom(entry))
    assert parsed.npics == entry["frames"]
    with R.DeviceContext(*_geom(entry), slots=parsed.npics) as ctx:
        ctx.upload_es(scan)
        mbs, coefs = ctx.download_records()
        assert mbs.tobytes() == parsed.mbs.tobytes()
        assert coefs.tobytes() == parsed.coefs.tobytes()
        ctx.decode()
        ctx.synchronize()
        assert [yuv_md5(ctx.download(int(d))) for d in parsed.display] == entry["md5"]
    with R.DeviceContext(*_geom(entry), slots=parsed.npics) as ctx:  # the same batch from host records
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        assert [yuv_md5(ctx.download(int(d))) for d in parsed.display] == entry["md5"]


@pytest.mark.parametrize("entry", NEGATIVE, ids=[e["name"] for e in NEGATIVE])
def test_out_of_contract_streams_are_rejected_with_the_hosts_status_and_reason(entry):
    es = _read(entry)
    with pytest.raises(_lib.Mp2vgError) as host:
        R.Parsed(es, *_geom(entry), threads=1)
    assert host.value.status == entry["status"] and entry["reason"] in str(host.value)
    with pytest.raises(_lib.Mp2vgError) as dev:
        scan = R.Scan(es, *_geom(entry))  # picture-level reasons are the scan's own
        with R.DeviceContext(*_geom(entry), slots=scan.npics) as ctx:
            ctx.upload_es(scan)
    assert dev.value.status == host.value.status
    assert _detail(str(dev.value)) == _detail(str(host.value))
