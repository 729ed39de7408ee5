"""Host side of the float32 matmul precision levels (ops.set_float32_matmul_precision, mtlssl_conv2d_set_fp32_engine
modes 0..3): names, the C ABI's mode register, the environment variable's unchanged meaning and the launchers' flag.
Needs the built library, no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ("highest", "split", "high", "medium")


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    prev = ops.set_fp32_engine(-1)
    yield ops
    ops.set_fp32_engine(prev)


def test_names_and_modes_round_trip_through_the_c_abi(ops):
    assert ops.FP32_ENGINES == dict(zip(NAMES, range(4)))
    ops.set_fp32_engine(0)
    prev = "highest"
    for name in NAMES + ("highest",):
        assert ops.set_float32_matmul_precision(name) == prev          # returns the previous NAME
        assert ops.get_float32_matmul_precision() == name
        assert ops.set_fp32_engine(-1) == ops.FP32_ENGINES[name]       # the C ABI's register holds the mode
        prev = name
    for name, mode in ops.FP32_ENGINES.items():                        # and the other way: set by mode, read by name
        ops.set_fp32_engine(mode)
        assert ops.get_float32_matmul_precision() == name


def test_unknown_name_raises_and_names_the_four(ops):
    ops.set_float32_matmul_precision("high")
    for bad in ("bf16", "HIGH", "", None, 2):
        with pytest.raises(ValueError) as e:
            ops.set_float32_matmul_precision(bad)
        assert all(n in str(e.value) for n in NAMES)
        assert ops.get_float32_matmul_precision() == "high"            # and leaves the level alone


def test_other_modes_only_query(ops):
    for held in (0, 1, 2, 3):
        ops.set_fp32_engine(held)
        for other in (7, 4, -1, -2, 1 << 20):
            assert ops.set_fp32_engine(other) == held
        assert ops.set_fp32_engine(-1) == held


def test_engine_launches_reports_four_counters_and_resets(ops):
    c = ops.engine_launches(reset=True)
    assert list(c) == ["native", "six", "three", "one"] and all(isinstance(v, int) and v >= 0 for v in c.values())
    assert ops.engine_launches() == dict.fromkeys(c, 0)                # nothing launched since the reset


@pytest.mark.parametrize("value,want", [("high", "highest"), ("3", "highest"), ("split", "split")])
def test_environment_variable_keeps_its_meaning(ops, value, want):
    """MTLSSL_FP32_ENGINE: split / 1 select the six-product engine, anything else the native one; the reduced levels
    are not reachable from the environment."""
    env = dict(os.environ)
    env.pop("MTLSSL_FP32_ENGINE", None)
    if value is not None:
        env["MTLSSL_FP32_ENGINE"] = value
    r = subprocess.run([sys.executable, "-c", "from mtl_ssl_amd import ops; print(ops.get_float32_matmul_precision())"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == want


def test_launchers_parse_the_flag_and_refuse_a_bad_value(ops, capsys):
    from mtl_ssl_amd import eval as evaluate
    from mtl_ssl_amd import train
    assert train.FLOAT32_MATMUL_PRECISIONS == tuple(ops.FP32_ENGINES)
    need = ["--checkpoint_dir=a", "--pipeline_config_path=b"]
    assert train._flags([]).float32_matmul_precision is None and evaluate._flags(need).float32_matmul_precision is None
    for name in NAMES:
        assert train._flags(["--float32_matmul_precision=" + name]).float32_matmul_precision == name
        assert evaluate._flags(need + ["--float32_matmul_precision", name]).float32_matmul_precision == name
    for parse in (lambda a: train._flags(a), lambda a: evaluate.main(need + a)):
        with pytest.raises(SystemExit) as e:
            parse(["--float32_matmul_precision=bf16"])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert all(n in err for n in NAMES)


def test_trainer_and_detector_take_the_keyword_last():
    import inspect
    from mtl_ssl_amd import inference, trainer
    for fn in (trainer.train, trainer.Trainer.__init__, inference.Detector.__init__, inference.Detector.from_export):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "float32_matmul_precision" and params[-1].default is None, fn
