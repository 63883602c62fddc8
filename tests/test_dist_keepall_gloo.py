"""CPU, world_size 2 over gloo: the torch transport of the chunk-record feature exchange (dist.allgather_feature_chunk_records), the way
keep-all frames (up to 32 768 keypoints) travel between ranks.  Ragged record counts: rank 0 holds frames of 1, 16 and 2 chunks, rank 1
none.  The records are laid out here on the host exactly as mi355_pack_feature_chunks_dev lays them out (the GPU side of the same layout is
tests/test_gpu_feature_chunks.py); every header and payload row must land where it was sent and every frame reassemble from its chunks."""
import os
import socket
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = textwrap.dedent("""
    import sys
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, %r)
    import imagemosaicing_amd as im
    from imagemosaicing_amd import dist as md

    REC, ROWS, KPB = im.FEATURE_RECORD_BYTES, im.FEATURE_CHUNK_ROWS, im.KEYPOINT.itemsize

    def frame(img_id, n):
        rng = np.random.default_rng(1000 + img_id)
        kp = rng.integers(0, 256, (n, KPB), dtype=np.uint8)
        d8 = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        return kp, d8

    def pack(img_id, n, w, h):
        kp, d8 = frame(img_id, n)
        nc = max(1, -(-n // ROWS))
        hdr = np.zeros(nc, im.FEATURE_CHUNK_HEADER)
        pay = np.zeros((nc, REC), np.uint8)
        for c in range(nc):
            r0 = c * ROWS
            rows = max(0, min(ROWS, n - r0))
            hdr[c] = (img_id, n, w, h, c, nc, r0, rows)
            pay[c, :rows * KPB] = kp[r0:r0 + rows].reshape(-1)
            pay[c, ROWS * KPB:ROWS * KPB + rows * 128] = d8[r0:r0 + rows].reshape(-1)
        return hdr, pay

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    frames = {0: [(10, 1500), (11, 32768), (12, 2049)], 1: []}        # 1 + 16 + 2 chunk records on rank 0, none on rank 1
    mine = [pack(i, n, 1000, 750) for i, n in frames[rank]]
    hdr = np.concatenate([m[0] for m in mine]) if mine else np.zeros(0, im.FEATURE_CHUNK_HEADER)
    pay = torch.from_numpy(np.concatenate([m[1] for m in mine])) if mine else torch.zeros((0, REC), dtype=torch.uint8)
    assert len(hdr) == (19 if rank == 0 else 0)
    hdrs, gp, counts = md.allgather_feature_chunk_records(hdr, pay)
    assert counts == [19, 0], counts
    assert gp.shape == (2, 19, REC) and gp.dtype == torch.uint8
    assert len(hdrs[0]) == 19 and len(hdrs[1]) == 0 and hdrs[0].dtype == im.FEATURE_CHUNK_HEADER
    # headers and payload rows land exactly where rank 0 put them, on both ranks
    want = [pack(i, n, 1000, 750) for i, n in frames[0]]
    want_h = np.concatenate([m[0] for m in want]); want_p = np.concatenate([m[1] for m in want])
    assert np.array_equal(hdrs[0].view(np.uint8), want_h.view(np.uint8))
    assert np.array_equal(gp[0].numpy(), want_p)
    # every frame reassembles from its chunks
    g = gp[0].numpy()
    for img_id, n in frames[0]:
        sel = np.flatnonzero(hdrs[0]["img_id"] == img_id)
        assert len(sel) == max(1, -(-n // ROWS)) and (hdrs[0]["n_kp"][sel] == n).all()
        sel = sel[np.argsort(hdrs[0]["chunk"][sel])]
        assert hdrs[0]["chunk"][sel].tolist() == list(range(len(sel)))
        kp = np.concatenate([g[k, :int(hdrs[0]["rows"][k]) * KPB].reshape(-1, KPB) for k in sel])
        d8 = np.concatenate([g[k, ROWS * KPB:ROWS * KPB + int(hdrs[0]["rows"][k]) * 128].reshape(-1, 128) for k in sel])
        kp0, d80 = frame(img_id, n)
        assert np.array_equal(kp, kp0) and np.array_equal(d8, d80), img_id
        for k in sel:                                  # zeros beyond the chunk's rows, in both parts of the record
            rows = int(hdrs[0]["rows"][k])
            assert not g[k, rows * KPB:ROWS * KPB].any() and not g[k, ROWS * KPB + rows * 128:].any()
    if rank == 0:
        print("KEEPALL_GLOO_OK", counts)
    dist.destroy_process_group()
""")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_chunk_records_ragged_counts_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % ROOT)
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "KEEPALL_GLOO_OK" in r.stdout
