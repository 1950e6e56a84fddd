"""GPU: one stream handle on two streams.  Every stream block has a "two handles, two streams" test; here ONE handle
runs input A on stream 1 and at once a different input B on stream 2, so the second run takes the handle's wait for
the first run's event (StreamHandle::begin in csrc/stream_capi.cpp: the runs share the handle's scratch).  Both outputs,
and the second run's counters and resume position, are the block's sequential reference's (tests/*_ref.py).  A race
may go unseen, so this cannot prove the wait; it pins that the path runs and gives the right bytes.

The inputs are the sizes of the blocks' own three-tile tests, so more than one scan tile of scratch is live."""
import numpy as np
import pytest

import dvbt2ll

pytestmark = pytest.mark.gpu


class Block:
    """handle: the one handle; launch(dev_input, out_ptr, cap, stream): its run_device with flush; inputs: two host
    inputs; refs: their reference results; caps: output capacities in units of `unit` bytes; units / out: the names of
    the counter of output units and of the reference's output field"""
    def __init__(self, handle, launch, upload, inputs, refs, caps, unit, units, out):
        self.handle, self.launch, self.upload, self.inputs, self.refs = handle, launch, upload, inputs, refs
        self.caps, self.unit, self.units, self.out = caps, unit, units, out


def _pdus_dev(x):
    import torch
    pdu, off = x
    return torch.from_numpy(pdu.copy()).cuda(), torch.from_numpy(off.view(np.int32).copy()).cuda()


def _pdu_block(enc, R, lists, ref, bound, unit=188, units="ts_packets", out="ts"):
    inputs = [R.pack(p) for p in lists]

    def launch(d, out_ptr, cap, stream):
        enc.run_device(d[0].data_ptr(), d[0].numel(), d[1].data_ptr(), d[1].numel() - 1, out_ptr, cap, flush=True,
                       stream=stream)
    return Block(enc, launch, _pdus_dev, inputs, [ref(pdu, off) for pdu, off in inputs],
                 [bound(len(pdu), len(off) - 1) for pdu, off in inputs], unit, units, out)


def _spanning(C, n, seed, tile, long=300):
    """n PDUs of 1 .. 40 bytes with a long one on each tile's last slot, as the blocks' own tile tests have them"""
    pdus = C.mixed(n, seed)
    for t in range(tile - 1, n, tile):
        pdus[t] = C.ip(long, t)
    return pdus


def _sizes(lists):
    return dict(max_pdu_bytes=max(sum(len(p) for p in ps) for ps in lists), max_pdus=max(len(ps) for ps in lists))


def ule():
    import ule_cases as C
    import ule_ref as R
    lists = [_spanning(C, 3 * 512 + 7, 11, 512), _spanning(C, 2 * 512 + 40, 12, 512)]
    enc = dvbt2ll.UleEncapsulator(pid=C.PID, dest=R.MAC, **_sizes(lists))
    return _pdu_block(enc, R, lists, lambda p, o: R.encap(p, o, pid=C.PID, flush=True, crc=R.crc32_table),
                      enc.packet_bound)


def mpe():
    import mpe_cases as C
    import mpe_ref as R
    lists = [_spanning(C, 3 * 512 + 7, 11, 512), _spanning(C, 2 * 512 + 40, 12, 512)]
    enc = dvbt2ll.MpeEncapsulator(pid=C.PID, mac_from_dest=True, **_sizes(lists))
    return _pdu_block(enc, R, lists, lambda p, o: R.encap(p, o, pid=C.PID, mac_mode=1, flush=True, crc=R.crc32_table),
                      enc.packet_bound)


def mpefec():
    import mpefec_cases as C
    import mpefec_ref as R
    # rows 256, three data columns, four RS columns, datagrams of 20 .. 40 bytes: 25 and 23 frames, whose 719 and 644
    # sections are more than one tile of 512 (the reference's Reed-Solomon columns take 15 ms a frame: no more frames)
    lists = [C.small_frames(512 + 107, 11, 20, 40), C.small_frames(512 + 40, 12, 20, 40)]
    enc = dvbt2ll.MpeFecEncapsulator(pid=C.PID, rows=256, data_columns=3, rs_columns=4, max_frames=64, **_sizes(lists))
    return _pdu_block(enc, R, lists, lambda p, o: R.encap(p, o, rows=256, D=3, K=4, pid=C.PID, mac=enc.mac, mac_mode=0,
                                                          packing=1, max_frames=64, flush=True), enc.packet_bound)


def gse():
    import gse_cases as C
    import gse_ref as R
    kbch, label = 7032, C.LABELS[2]
    long = 2 * C.D_of(kbch) + 50
    lists = [_spanning(C, 3 * 256 + 7, 11, 256, long), _spanning(C, 2 * 256 + 40, 12, 256, long)]
    enc = dvbt2ll.GseEncapsulator(kbch=kbch, label=label, **_sizes(lists))
    return _pdu_block(enc, R, lists, lambda p, o: R.encap(p, o, kbch=kbch, label=label, flush=True, crc=R.crc32_table),
                      enc.frame_bound, unit=enc.Lb, units="bbframes", out="bb")


def modeadapt():
    import torch
    import modeadapt_cases as C
    import modeadapt_ref as R
    # 2200 packets (three scan tiles of 1024) and 2100 others, null runs across the tile boundaries
    inputs = [C.two_tile_stream(), C.stream([(C.PID_A, 500), (C.PID_NULL, 700), (C.PID_A, 900)], seed=5)]
    ad = dvbt2ll.ModeAdapter(kbch=C.KBCH_SHORT14, max_ts_bytes=max(len(ts) for ts in inputs))

    def launch(d, out_ptr, cap, stream):
        ad.run_device(d.data_ptr(), d.numel(), out_ptr, cap, flush=True, stream=stream)
    return Block(ad, launch, lambda ts: torch.from_numpy(ts.copy()).cuda(), inputs,
                 [R.adapt(ts, C.KBCH_SHORT14, flush=True) for ts in inputs], [len(ts) // ad.D + 2 for ts in inputs],
                 ad.L, "bbframes", "bbframes")


@pytest.mark.parametrize("make", [ule, mpe, mpefec, gse, modeadapt])
def test_one_handle_two_streams(gpu, make):
    import torch
    b = make()
    assert all(ref.counters[b.units] > 0 for ref in b.refs)
    assert not np.array_equal(getattr(b.refs[0], b.out), getattr(b.refs[1], b.out))
    dev = [b.upload(x) for x in b.inputs]
    outs = [torch.zeros(cap * b.unit, dtype=torch.uint8, device="cuda") for cap in b.caps]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream and 0 not in [s.cuda_stream for s in streams]
    torch.cuda.synchronize()
    for k in range(2):
        b.launch(dev[k], outs[k].data_ptr(), b.caps[k], streams[k].cuda_stream)
    res = b.handle.result()        # waits for the second run's event
    # the second run waited for the first one's event, so stream 1 has nothing left to do
    assert streams[0].query(), "the first run was still going when the second had finished"
    for s in streams:
        s.synchronize()
    for k in range(2):
        want = getattr(b.refs[k], b.out)
        np.testing.assert_array_equal(outs[k].cpu().numpy()[:len(want)], want, err_msg="run %d" % k)
    assert tuple(res.resume) == tuple(b.refs[1].resume), (res.resume, b.refs[1].resume)
    assert res.counters == b.refs[1].counters, (res.counters, b.refs[1].counters)
