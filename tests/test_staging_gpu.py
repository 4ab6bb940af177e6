"""The one staging protocol of the policy handle (arp_amd/csrc/arp_dt.hip: stage_slot under stage_sync / stage_async), for every kind of batch:

* a refused synchronous batch of any kind leaves the selected slot -- the synchronous one or a prefetch slot -- selected and its batch usable;
* a prefetch slot that was uploaded and encoded ahead may be refilled without ever being selected: the new upload waits for the encoder pass;
* host encodings, host frames, index batches and (row, goal row) pairs through prefetch_to_device equal their synchronous feed.

Every comparison is bitwise: the same kernels on the same bytes, staged another way.  The set is tests/test_dataset_gpu.py's 24 rows, read with window 4."""
import numpy as np
import pytest

from test_dataset_gpu import TINY_ENC, _data
from test_dataset_gpu import _host_batch as _frames_batch
from test_gcbc_dataset_gpu import _host_batch as _goal_batch
from test_gcbc_gpu import SMALL_ENC

pytestmark = pytest.mark.gpu

W = 4
ROWS3, ROWS2 = [0, 23, 5], [10, 3]            # B = 3: a one-row trajectory, the last row, a long one; B = 2
GOALS3, GOALS2 = [0, 23, 9], [12, 9]
STEPS = [(ROWS3, GOALS3), (ROWS2, GOALS2), ([8, 20, 13], [9, 22, 20])]  # three steps: slots 0 (B = 3), 1 (B = 2), 0

_CACHE = {}


def _pd():
    if "pd" not in _CACHE:
        from arp_amd.dataset import ProcgenDataset
        _CACHE["pd"] = ProcgenDataset(dict(_data(64)[0]), W, env_name="coinrun")
    return _CACHE["pd"]


def _frames(idx):
    from arp_amd import dataset
    return _frames_batch(_pd(), idx, dataset.default_lut())


def _pairs(idx, gidx):
    from arp_amd import dataset
    return _goal_batch(_pd(), idx, dataset.default_lut(), goal_index=gidx)


def _encodings(idx, tokens, dim, seed=9):
    """the labels of rows idx under random encodings"""
    b = _frames(idx)
    return {"image": {"ob": np.random.default_rng(seed + idx[0]).standard_normal((len(idx), W, tokens, dim)).astype(np.float32)}, "action": b["action"], "rtg": b["rtg"]}


class _Handle:
    """A trainer behind its own frozen encoder, and (dataset=True) the device-resident set."""

    def __init__(self, model, mode, dataset=False):
        from arp_amd import dataset as D, m3ae, synth_policy as S
        from arp_amd.train import PolicyConfig, TrainState
        from oracle import m3ae_np as M
        enc_kw = SMALL_ENC if model == "GCBC" else TINY_ENC
        ecfg = m3ae.EncoderConfig(**enc_kw)
        kw = dict(emb=64, depth=2, heads=4, window=W, enc_dim=ecfg.width)
        self.cfg = PolicyConfig(**kw, enc_tokens=ecfg.gc_tokens, model="GCBC") if model == "GCBC" else PolicyConfig(**kw, enc_tokens=ecfg.tokens, lambda_ret=0.5)
        self.enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(**enc_kw), seed=5), mode=mode)
        self.state = TrainState.create(self.cfg, S.policy_params(self.cfg, seed=6), mode=mode)
        self.tr = self.state.trainer
        self.tr.attach_encoder(self.enc)
        self.ds = D.DeviceDataset.load(_pd()) if dataset else None
        if dataset:
            self.tr.attach_dataset(self.ds)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.tr.close()
        if self.ds is not None:
            self.ds.close()
        self.enc.close()


def _same_forward(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("model", ["ARPDT", "GCBC"])
def test_a_refused_synchronous_batch_leaves_the_selected_slot(gpu_lib, model):
    """One refused call of each kind -- an action id out of range, an index outside the set: host-side checks, nothing is launched -- with the
    synchronous slot selected (B = 3), then with prefetch slot 0 selected (B = 2): forward() reads what it read before, bit for bit."""
    from arp_amd._ffi import ArpError
    n = _pd().n_rows
    with _Handle(model, "f32", dataset=True) as h:
        tr = h.tr
        E = _encodings(ROWS3, h.cfg.enc_tokens, h.cfg.enc_dim)
        F = _frames(ROWS3) if model == "ARPDT" else _pairs(ROWS3, GOALS3)
        bad = F["action"].copy()
        bad[1, 2] = h.cfg.n_actions

        def refused():
            with pytest.raises(ArpError, match="action id out of range"):  # encodings
                tr.set_batch(E["image"]["ob"], bad, E["rtg"]["ob"])
            if model == "ARPDT":
                with pytest.raises(ArpError, match="action id out of range"):  # frames
                    tr.set_batch_images(F["image"]["ob"], bad, F["rtg"]["ob"])
                with pytest.raises(ArpError, match=r"index .* \(batch position 1\) is outside"):  # index
                    tr.set_batch_indices([0, n, 1])
            else:
                with pytest.raises(ArpError, match="action id out of range"):  # frames + goals
                    tr.set_batch_images(F["image"]["ob"], bad, goals=F["goal"]["ob"])
                with pytest.raises(ArpError, match=r"goal index .* \(batch position 1\) is outside"):  # index pairs
                    tr.set_batch_index_pairs(ROWS3, [0, n, 1])
                with pytest.raises(ArpError, match=r"index .* \(batch position 2\) is outside"):
                    tr.set_batch_index_pairs([0, 1, -1], GOALS3)

        if model == "ARPDT":
            tr.set_batch_images(F["image"]["ob"], F["action"], F["rtg"]["ob"])
        else:
            tr.set_batch_images(F["image"]["ob"], F["action"], goals=F["goal"]["ob"])
        first = tr.forward()
        assert first["action_pred"].shape[0] == 3 and np.isfinite(first["loss"])
        refused()
        _same_forward(tr.forward(), first)

        if model == "ARPDT":
            f2 = _frames(ROWS2)
            tr.upload_async(0, f2["image"]["ob"], f2["action"], f2["rtg"]["ob"], images=True)
        else:
            tr.upload_index_pairs_async(0, ROWS2, GOALS2)
        tr.select(0)
        second = tr.forward()
        assert second["action_pred"].shape[0] == 2 and second["loss"] != first["loss"]
        refused()
        _same_forward(tr.forward(), second)
        assert np.isfinite(tr.train_step(1e-3)["loss"])  # and the slot still trains


@pytest.mark.parametrize("second", ["frames", "encodings"])
def test_an_unconsumed_encoded_ahead_slot_can_be_refilled(gpu_lib, monkeypatch, second):
    """Frames into slot 0, encode_ahead(0), then ANOTHER batch into slot 0 -- frames, or encodings that land in the very buffer the encoder pass writes --
    without a select in between: the upload waits for the pass.  The step on the slot equals the step on the same batch staged synchronously on a twin."""
    monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)
    monkeypatch.delenv("ARP_DT_ENC_EAGER", raising=False)
    out = []
    for feed in ("refill", "sync"):
        with _Handle("ARPDT", "f16") as h:
            tr = h.tr
            x = _frames(ROWS3)
            y = _frames(ROWS2) if second == "frames" else _encodings(ROWS2, h.cfg.enc_tokens, h.cfg.enc_dim)
            if feed == "refill":
                tr.upload_async(0, x["image"]["ob"], x["action"], x["rtg"]["ob"], images=True)
                tr.encode_ahead(0)
                tr.upload_async(0, y["image"]["ob"], y["action"], y["rtg"]["ob"], images=second == "frames")
                tr.select(0)
            elif second == "frames":
                tr.set_batch_images(y["image"]["ob"], y["action"], y["rtg"]["ob"])
            else:
                tr.set_batch(y["image"]["ob"], y["action"], y["rtg"]["ob"])
            out.append((tr.train_step(1e-3), tr.get_params()))
    (aux_a, pa), (aux_b, pb) = out
    assert np.isfinite(aux_a["loss"]) and aux_a == aux_b, (aux_a, aux_b)
    assert all(np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)) for k in pa)


def _step_batches(kind, cfg):
    if kind == "encodings":
        return [_encodings(i, cfg.enc_tokens, cfg.enc_dim) for i, _ in STEPS]
    if kind == "frames":
        return [_frames(i) for i, _ in STEPS]
    if kind == "index":
        return [{"index": np.asarray(i, np.int64)} for i, _ in STEPS]
    return [{"index": np.asarray(i, np.int64), "goal_index": np.asarray(g, np.int64)} for i, g in STEPS]


@pytest.mark.parametrize("kind", ["encodings", "frames", "index", "index_pairs"])
def test_every_kind_prefetched_equals_its_synchronous_feed(gpu_lib, monkeypatch, kind):
    """Three steps through prefetch_to_device (slots 0, 1, 0; frames are encoded ahead) against the same batches staged synchronously by the step function."""
    from arp_amd.train import DeviceBatch, create_train_step, prefetch_to_device
    monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)
    monkeypatch.delenv("ARP_DT_ENC_EAGER", raising=False)
    out = []
    for feed in ("prefetch", "sync"):
        with _Handle("GCBC" if kind == "index_pairs" else "ARPDT", "f16", dataset=kind.startswith("index")) as h:
            fn = create_train_step(h.cfg, lambda step: 1e-3, h.cfg.weight_decay)
            state, auxes, slots = h.state, [], []
            batches = _step_batches(kind, h.cfg)
            for b in prefetch_to_device(iter(batches), 2, h.tr) if feed == "prefetch" else batches:
                if feed == "prefetch":
                    assert isinstance(b, DeviceBatch)
                    slots.append(b.slot)
                state, aux, _ = fn(state, b, None)
                auxes.append(aux)
            assert slots == ([0, 1, 0] if feed == "prefetch" else [])
            out.append((auxes, h.tr.get_params()))
    (aux_a, pa), (aux_b, pb) = out
    assert len(aux_a) == 3 and all(np.isfinite(a["loss"]) for a in aux_a)
    assert aux_a == aux_b, (aux_a, aux_b)
    assert all(np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)) for k in pa)
