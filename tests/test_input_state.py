"""CPU tests of stopping and continuing the input stream (InputPipeline.state / restore, the input states in the
state file, their gathering over data-parallel ranks). The arbiter of a continued stream is the uninterrupted one:
`input_reader.batches` with the same arguments, its first k batches skipped. Every comparison is equality."""
import json
import os

import numpy as np
import pytest

from mtl_ssl_amd import checkpoint, config
from mtl_ssl_amd import input_pipeline as P
from mtl_ssl_amd import input_reader as R
from tests.test_input_pipeline import FLIP2, K, SHAPES, _assert_same, _example, _resized

PHOTOMETRIC = config.parse_pipeline_config("""train_config {
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 } }
  data_augmentation_options { random_adjust_brightness { max_delta: 0.3 } }
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 } }
  data_augmentation_options { random_black_patches { max_black_patches: 3 probability: 0.7 size_to_image_ratio: 0.2 } }
}""").train_config.data_augmentation_options
CROP = config.parse_pipeline_config("""train_config {
  data_augmentation_options { random_crop_image { min_object_covered: 0.0 min_area: 0.3 random_coef: 0.3 } }
}""").train_config.data_augmentation_options
# the stream the issue names for the "snapshot is non-trivial" check; most other tests use it too
LOOPED = dict(batch_size=2, augmentation_options=FLIP2, shuffle_buffer=3, max_pending=5, loop=True, resized_shape=_resized)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """The 11 records in two files of tests/test_input_pipeline.py."""
    d = tmp_path_factory.mktemp("state")
    rng = np.random.RandomState(3)
    paths = []
    for part, shapes in enumerate((SHAPES[:6], SHAPES[6:])):
        p = str(d / ("part%d.record" % part))
        R.write_tfrecord(p, [_example(rng, 10 * part + i, h, w, boxes=(i != 2)) for i, (h, w) in enumerate(shapes)])
        paths.append(p)
    return paths


def _dumps(state):
    return json.dumps(state, sort_keys=True)


def _reference(paths, n, seed=7, **kw):
    """The first n batches of the uninterrupted stream (all of a shorter one)."""
    out = []
    for b in R.batches(paths, K, rng=np.random.RandomState(seed), **kw):
        out.append(b)
        if len(out) == n:
            break
    return out


def _take(pipe, n):
    return [next(pipe) for _ in range(n)]


def _stop_and_continue(paths, k, n, workers=2, seed=7, **kw):
    """k batches, state() through JSON, close; a new pipeline (another RandomState, which restore must overwrite)
    continues for n batches. -> (the n batches, the state as a JSON string)."""
    with P.InputPipeline(paths, K, rng=np.random.RandomState(seed), num_workers=workers, prefetch=2, **kw) as pipe:
        _take(pipe, k)
        text = json.dumps(pipe.state())
    with P.InputPipeline(paths, K, rng=np.random.RandomState(seed + 100), num_workers=workers, prefetch=3, **kw) as pipe:
        pipe.restore(json.loads(text))
        return _take(pipe, n), text


ROUND_TRIPS = {
    # id: (k, n, workers, arguments). Without loop the 11 records end; k + n stays inside the stream there.
    "b1": (3, 4, 2, dict(batch_size=1, augmentation_options=FLIP2, resized_shape=_resized, max_pending=3)),
    "b2": (2, 3, 2, dict(batch_size=2, augmentation_options=FLIP2, resized_shape=_resized, max_pending=3)),
    "b3": (1, 2, 2, dict(batch_size=3, augmentation_options=FLIP2, resized_shape=_resized, max_pending=3)),
    "shuffle0_loop": (4, 5, 2, dict(LOOPED, shuffle_buffer=0)),                 # 4 + 5 batches of 2 cross the 11 records
    "shuffle3_loop": (5, 6, 2, LOOPED),
    "rank0": (2, 4, 2, dict(LOOPED, rank=0, world=2, shuffle_buffer=4, max_pending=4)),
    "rank1": (2, 4, 2, dict(LOOPED, rank=1, world=2, shuffle_buffer=4, max_pending=4)),
    "photometric": (3, 5, 2, dict(LOOPED, augmentation_options=PHOTOMETRIC)),
    "geometric": (3, 6, 2, dict(LOOPED, augmentation_options=CROP, geometric=True)),
    "workers1": (3, 6, 1, LOOPED),
    "workers3": (3, 6, 3, LOOPED),
}


@pytest.mark.parametrize("case", sorted(ROUND_TRIPS))
def test_round_trip_continues_the_uninterrupted_stream(records, case):
    k, n, workers, kw = ROUND_TRIPS[case]
    want = _reference(records, k + n, **kw)
    assert len(want) == k + n
    if kw.get("loop"):
        assert sum(len(b["filename"]) for b in want) * kw.get("world", 1) > len(SHAPES)      # crosses the epoch
    got, _ = _stop_and_continue(records, k, n, workers, **kw)
    _assert_same(got, want[k:])


def test_state_holds_bucketed_items_and_does_not_depend_on_timing(records):
    """After every one of the first 14 batches of this stream some examples wait in buckets (a snapshot of empty
    buckets would prove nothing), and the state is the same text whatever the worker count and the prefetch depth."""
    texts = {}
    for workers, prefetch in ((1, 1), (3, 4)):
        with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=workers, prefetch=prefetch,
                             **LOOPED) as pipe:
            texts[workers] = [_dumps(pipe.state())]
            for _ in range(14):
                next(pipe)
                texts[workers].append(_dumps(pipe.state()))
    assert texts[1] == texts[3]
    for k in range(1, 15):
        st = json.loads(texts[1][k])
        waiting = sum(len(b["items"]) for b in st["buckets"])
        assert waiting >= 1 and waiting == st["pending"] and st["batches"] == k and not st["replay"]
        assert all(len(it["draws"]) == 2 and len(it["record"]) == 4 for b in st["buckets"] for it in b["items"])
        assert st["rng"][0] == "MT19937" and len(st["rng"][1]) == 624 and len(st["shuffle"]) == 3
    start = json.loads(texts[1][0])
    assert start["batches"] == 0 and start["items"] == 0 and start["buckets"] == [] and start["shuffle"] == []
    assert start["cursor"] == {"pass": 0, "file": 0, "record": 0, "i": 0}
    assert len({t for t in texts[1]}) == 15


def test_restored_pipeline_reports_the_state_it_was_given(records):
    with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=2, **LOOPED) as pipe:
        _take(pipe, 4)
        st = pipe.state()
    with P.InputPipeline(records, K, num_workers=1, state=json.loads(json.dumps(st)), **LOOPED) as pipe:
        assert _dumps(pipe.state()) == _dumps(st)


def test_chain_of_restores(records):
    """restore -> 2 batches -> state -> restore -> continue: equal to the uninterrupted stream, and every state on
    the way is the text the uninterrupted pipeline gives after as many batches."""
    want = _reference(records, 12, **LOOPED)
    with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=2, **LOOPED) as pipe:
        texts = [_dumps(pipe.state())]
        for _ in range(12):
            next(pipe)
            texts.append(_dumps(pipe.state()))
    st, got, at = json.loads(texts[3]), [], 3
    for n in (2, 2, 5):
        with P.InputPipeline(records, K, num_workers=2, prefetch=2, state=st, **LOOPED) as pipe:
            got += _take(pipe, n)
            at += n
            assert _dumps(pipe.state()) == texts[at]
            st = json.loads(json.dumps(pipe.state()))
    _assert_same(got, want[3:12])


@pytest.mark.parametrize("back", [5, 2, 1, 0])
def test_non_looping_stream_ends_with_the_same_remainder(records, back):
    """Stopped `back` batches before the end (for back < 4 inside the leftovers that drop_remainder=False hands out in
    key order): the continuation is the rest, then StopIteration."""
    kw = dict(batch_size=2, augmentation_options=FLIP2, resized_shape=_resized, shuffle_buffer=3, max_pending=6)
    want = _reference(records, None, **kw)
    assert [len(b["filename"]) for b in want][-5:] == [2, 1, 1, 1, 1]          # the stream ends with four leftovers
    k = len(want) - back
    with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=2, **kw) as pipe:
        _take(pipe, k)
        st = json.loads(json.dumps(pipe.state()))
    assert st["exhausted"] == (back < 4)                     # a mark inside the leftovers says so; one before them does not
    with P.InputPipeline(records, K, num_workers=2, state=st, **kw) as pipe:
        got = list(pipe)
        with pytest.raises(StopIteration):
            next(pipe)
    _assert_same(got, want[k:])


def test_mismatch_names_the_field(records, tmp_path):
    with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=1, **LOOPED) as pipe:
        _take(pipe, 2)
        st = json.loads(json.dumps(pipe.state()))
    assert issubclass(P.InputStateMismatch, ValueError)

    def refused(field, paths=records, **changed):
        with P.InputPipeline(paths, K, num_workers=1, **dict(LOOPED, **changed)) as other:
            with pytest.raises(P.InputStateMismatch, match=field) as e:
                other.restore(st)
            assert e.value.field == field
            assert other.state()["items"] == 0                     # a refused state leaves the pipeline as it was
    refused("batch_size", batch_size=3)
    refused("paths", paths=records[::-1])
    refused("options", augmentation_options=FLIP2[:1])
    refused("world", world=2)
    refused("resized_shape", resized_shape=None)                   # the resize rule, through the recorded bucket keys
    # a record file of another size under the same name
    grown = str(tmp_path / "part0.record")
    rng = np.random.RandomState(3)
    R.write_tfrecord(grown, [_example(rng, i, 12, 16) for i in range(3)])
    with P.InputPipeline([grown], K, rng=np.random.RandomState(7), num_workers=1, **LOOPED) as pipe:
        next(pipe)
        small = pipe.state()
    R.write_tfrecord(grown, [_example(rng, i, 12, 16) for i in range(4)])
    with P.InputPipeline([grown], K, num_workers=1, **LOOPED) as other:
        with pytest.raises(P.InputStateMismatch, match="file_sizes"):
            other.restore(small)
    # not after the first batch
    with P.InputPipeline(records, K, num_workers=1, **LOOPED) as late:
        next(late)
        with pytest.raises(RuntimeError, match="before the first batch"):
            late.restore(st)


def test_host_generator_is_followed_batch_for_batch(records):
    """train.HostBatches(follow_state=True): the serial generator's batches untouched, and beside them the state the
    asynchronous pipeline reports after as many batches, which such a pipeline can continue; without follow_state there
    is no state and no second pipeline."""
    from mtl_ssl_amd import train
    kw = {k: v for k, v in LOOPED.items() if k not in ("batch_size", "augmentation_options")}
    want = _reference(records, 9, **LOOPED)
    with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=2, **LOOPED) as pipe:
        _take(pipe, 5)
        text = _dumps(pipe.state())
    host = train.HostBatches(records, K, 2, FLIP2, np.random.RandomState(7), "cpu", follow_state=True, **kw)
    try:
        _assert_same(_take(host, 5), want[:5])
        assert _dumps(host.state()) == text and not hasattr(host, "restore")
        with P.InputPipeline(records, K, num_workers=1, state=json.loads(json.dumps(host.state())), **LOOPED) as pipe:
            _assert_same(_take(pipe, 4), want[5:])
    finally:
        host.close()
    plain = train.record_batches("host", records, K, 2, FLIP2, np.random.RandomState(7), "cpu", {}, **kw)
    _assert_same(_take(plain, 2), want[:2])
    assert plain.state() is None and plain._shadow is None


# ---------------------------------------------------------------------------------------------------- the state file
def _tiny_store():
    from mtl_ssl_amd.params import ParamStore
    ps = ParamStore()
    ps.add("a/weights", (3, 2), "zeros")
    ps.add("a/moving_mean", (2,), "zeros", trainable=False)
    return ps.finalize("cpu", values={"a/weights": np.arange(6, dtype=np.float32).reshape(3, 2),
                                      "a/moving_mean": np.ones(2, np.float32)})


def test_state_file_carries_the_input_states(records, tmp_path):
    states = []
    for rank in (0, 1):
        with P.InputPipeline(records, K, rng=np.random.RandomState(7 + rank), num_workers=1, rank=rank, world=2,
                             **LOOPED) as pipe:
            _take(pipe, 2)
            states.append(pipe.state())
    ps = _tiny_store()
    path = str(tmp_path / "model.ckpt.npz")
    checkpoint.save(path, ps, 17, None, input_states=states)
    ck = np.load(path, allow_pickle=False)
    assert {k: ck[k].dtype for k in ck.files if k.startswith("input_state/rank")} == {
        "input_state/rank0": np.dtype(np.uint8), "input_state/rank1": np.dtype(np.uint8)}
    assert int(ck["input_state/world"]) == 2
    for k in ck.files:
        ck[k]                                                          # every array loads without pickle
    back = checkpoint.load_input_states(path)
    assert [_dumps(s) for s in back] == [_dumps(s) for s in states]
    fresh = _tiny_store()
    fresh.value("a/weights").zero_()
    assert checkpoint.load(path, fresh) == 17
    assert np.array_equal(fresh.value("a/weights").numpy(), ps.value("a/weights").numpy())
    plain = str(tmp_path / "plain.npz")
    checkpoint.save(plain, ps, 3)
    assert checkpoint.load_input_states(plain) is None and checkpoint.load(plain, fresh) == 3
    assert not [k for k in np.load(plain).files if k.startswith("input_state/")]


def test_restore_input_state_says_why_a_stream_starts_afresh(records, tmp_path):
    """trainer.restore_input_state, the resume step of trainer.train: the rank's own entry is restored; a file without
    input states, one saved by another number of ranks and a differently defined pipeline leave the stream at its first
    record and say so in one line."""
    from mtl_ssl_amd import trainer
    want = _reference(records, 6, **LOOPED)
    with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=1, **LOOPED) as pipe:
        _take(pipe, 2)
        st = pipe.state()
    ps, said = _tiny_store(), []
    one, two, none = (str(tmp_path / n) for n in ("one.npz", "two.npz", "none.npz"))
    checkpoint.save(one, ps, 2, None, input_states=[st])
    checkpoint.save(two, ps, 2, None, input_states=[st, st])
    checkpoint.save(none, ps, 2)
    with P.InputPipeline(records, K, num_workers=1, **LOOPED) as pipe:
        assert trainer.restore_input_state(pipe, one, 0, 1, say=said.append) and not said
        _assert_same(_take(pipe, 4), want[2:])
    for path, changed, why in ((none, {}, "holds no input state"), (two, {}, "saved by 2 rank(s), this run has 1"),
                               (one, dict(shuffle_buffer=4), "another shuffle_buffer")):
        del said[:]
        with P.InputPipeline(records, K, rng=np.random.RandomState(7), num_workers=1, **dict(LOOPED, **changed)) as pipe:
            assert not trainer.restore_input_state(pipe, path, 0, 1, say=said.append)
            assert len(said) == 1 and "restarts at its first record" in said[0] and why in said[0], said
            if not changed:
                _assert_same(_take(pipe, 2), want[:2])


# ------------------------------------------------------------------------------------- two gloo ranks on the CPU
def _rank_worker(rank, world, port, paths, path, out):
    import torch.distributed as dist
    from mtl_ssl_amd import trainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    kw = dict(LOOPED, rank=rank, world=world)
    with P.InputPipeline(paths, K, rng=np.random.RandomState(7 + rank), num_workers=1, **kw) as pipe:
        _take(pipe, 3)
        states = trainer.gather_input_states(pipe.state())
    if rank == 0:
        checkpoint.save(path, _tiny_store(), 3, None, input_states=states)
    else:
        assert states is None
    # the chief alone wishes to save; every rank learns it (and the failure code) in one all-reduce
    from mtl_ssl_amd.comm import GlooComm
    assert trainer.collective_step_verdict(GlooComm(), 2 * rank, rank == 0, "cpu") == (2, True)
    assert trainer.collective_step_verdict(GlooComm(), 0, False, "cpu") == (0, False)
    assert trainer.gather_input_states(None) is None               # a stream without state(): nothing to store
    dist.barrier()
    mine = checkpoint.load_input_states(path)[rank]
    with P.InputPipeline(paths, K, num_workers=1, state=mine, **kw) as pipe:
        got = _take(pipe, 4)
    want = _reference(paths, 7, seed=7 + rank, **kw)
    try:
        _assert_same(got, want[3:])
        out[rank] = "equal"
    except AssertionError as e:
        out[rank] = "differs: %s" % e
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_and_continue(records, tmp_path):
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    port = 29500 + ((os.getpid() + 500) % 1000)
    path = str(tmp_path / "model.ckpt.npz")
    mp.spawn(_rank_worker, args=(2, port, list(records), path, out), nprocs=2, join=True)
    assert dict(out) == {0: "equal", 1: "equal"}
    assert int(np.load(path, allow_pickle=False)["input_state/world"]) == 2
