"""batch["captions_per_image"] on the host: every refusal fires before anything touches a device (a model stub whose `_dev` fails the
test), and the regrouping of packed rows for the cross-attention beyond one tile (`group_packed_rows`).  No GPU needed."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _batch(n_img, n_cap, T=6, **extra):
    b = {"pixel_values": np.zeros((n_img, 8, 8, 3), np.float32), "input_ids": np.zeros((n_cap, T), np.int64),
         "attention_mask": np.ones((n_cap, T), np.int64), "decoder_input_ids": np.zeros((n_cap, T), np.int64)}
    b.update(extra)
    return b


class _Stub:
    """a model nothing may be asked of: the Trainer must refuse before it moves a tensor to the device"""
    store = None

    def __init__(self, fp8=False):
        self.engine = types.SimpleNamespace(fp8=fp8)

    def _dev(self, *a, **k):
        raise AssertionError("the batch was moved to the device before the refusal")

    @property
    def device(self):
        raise AssertionError("the model's device was asked for before the refusal")


def _trainer(fp8=False):
    from mic_amd import Trainer

    tr = Trainer.__new__(Trainer)  # no constructor: the stub has no store to lay out, and none of it is needed before the refusal
    tr.model = _Stub(fp8)
    tr.accumulate_steps, tr._micro, tr._cu_budget, tr.seed, tr.rank, tr.step = 1, 0, 0, 0, 0, 0
    tr.reducer = types.SimpleNamespace(step_stream=None)
    return tr


BAD = [
    ("integer >= 1", _batch(2, 4, captions_per_image=True)),
    ("integer >= 1", _batch(2, 2, captions_per_image=np.bool_(True))),
    ("integer >= 1", _batch(2, 4, captions_per_image=2.0)),
    ("integer >= 1", _batch(2, 4, captions_per_image="2")),
    ("integer >= 1", _batch(2, 4, captions_per_image=None)),
    ("integer >= 1", _batch(2, 4, captions_per_image=0)),
    ("integer >= 1", _batch(2, 4, captions_per_image=-2)),
    ("caption rows", _batch(2, 5, captions_per_image=2)),
    ("caption rows", _batch(2, 4, captions_per_image=3)),
    ("caption rows", _batch(2, 4)),                          # without the key: one caption row per image, as ever
    ("caption rows", _batch(2, 4, captions_per_image=1)),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_refusals_come_before_any_device_work(i):
    from mic_amd.train import check_captions_per_image

    word, b = BAD[i]
    with pytest.raises(ValueError, match=word):
        check_captions_per_image(b)
    tr = _trainer()
    for step in (tr.train_step, tr.eval_step):
        with pytest.raises(ValueError, match=word):
            step(b)


def test_fp8_gemms_refuse_more_than_one_caption_per_image():
    from mic_amd.train import check_captions_per_image

    b = _batch(2, 4, captions_per_image=np.int64(2))
    assert check_captions_per_image(b) == 2 and check_captions_per_image(_batch(3, 3)) == 1
    with pytest.raises(ValueError, match="gemm_dtype='fp8'"):
        check_captions_per_image(b, fp8=True)
    assert check_captions_per_image(_batch(2, 2, captions_per_image=1), fp8=True) == 1  # G = 1 is today's step, fp8 included
    tr = _trainer(fp8=True)
    for step in (tr.train_step, tr.eval_step):
        with pytest.raises(ValueError, match="gemm_dtype='fp8'"):
            step(b)
    # an accepted batch goes on to the device: the stub says so
    with pytest.raises(AssertionError, match="moved to the device"):
        _trainer().eval_step(b)


def test_engine_refuses_rows_that_do_not_divide_over_the_images():
    from mic_amd.engine import Engine

    eng = Engine.__new__(Engine)
    eng.fp8 = False
    assert eng._kv_group(6, None) == 1 and eng._kv_group(6, 6) == 1 and eng._kv_group(6, 2) == 3
    for images in (4, 0, -1, 12):
        with pytest.raises(ValueError):
            eng._kv_group(6, images)
    with pytest.raises(ValueError, match="group_packed_rows"):
        eng._kv_group(6, 2, pack=(None, None, 10))
    eng.fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        eng._kv_group(6, 2)
    assert eng._kv_group(6, 6) == 1


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_group_packed_rows_on_ragged_lengths(G):
    from mic_amd import group_packed_rows, packed_rows

    n_img, T = 3, 9
    rng = np.random.default_rng(G)
    ln = rng.integers(1, T + 1, n_img * G)
    ln[0], ln[-1], ln[1 % ln.size] = 1, T, 1           # length-1 captions and a full one among them
    mask = (np.arange(T)[None, :] < ln[:, None]).astype(np.int64)
    dec_in = rng.integers(4, 100, (n_img * G, T))
    q_off, q_len, ids, pos = packed_rows(mask, dec_in)
    goff, glen = group_packed_rows(q_off, q_len, G)
    assert goff.dtype == np.int32 and glen.dtype == np.int32 and goff.shape == glen.shape == (n_img,)
    assert int(glen.sum()) == int(q_len.sum()) == int(mask.sum())
    for i in range(n_img):
        mine = list(range(i * G, (i + 1) * G))
        assert goff[i] == q_off[mine[0]] and glen[i] == sum(int(q_len[b]) for b in mine)
        # one contiguous range: every caption of the image starts where the one before it ended, and the image ends where the next begins
        for a, b in zip(mine, mine[1:]):
            assert q_off[b] == q_off[a] + q_len[a]
        covered = np.concatenate([np.arange(q_off[b], q_off[b] + q_len[b]) for b in mine])
        assert np.array_equal(covered, np.arange(goff[i], goff[i] + glen[i]))
        if i + 1 < n_img:
            assert goff[i + 1] == goff[i] + glen[i]
    if G == 1:
        assert np.array_equal(goff, q_off) and np.array_equal(glen, q_len)


def test_group_packed_rows_refuses_what_it_cannot_group():
    from mic_amd import group_packed_rows

    with pytest.raises(ValueError):
        group_packed_rows([0, 3, 5], [3, 2, 4], 2)          # 3 sequences, groups of 2
    with pytest.raises(ValueError):
        group_packed_rows([0, 3], [3, 2], 0)
    with pytest.raises(ValueError, match="without gaps"):
        group_packed_rows([0, 4], [3, 2], 2)                # a gap between two captions: not one range
    off, ln = group_packed_rows(np.zeros(0, np.int32), np.zeros(0, np.int32), 2)
    assert off.size == 0 and ln.size == 0
