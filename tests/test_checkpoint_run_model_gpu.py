"""run_model --save_model / --load_model on the ML-1M fixture, d = 8, the
settings of test_cg_models_gpu.py without --use_cg: two epochs, save, then a
second process that loads and trains one more, against three epochs in one
process.  The resumed log has the one line "Epoch: 2, Timer" and its
"Validation Results" block says what the three-epoch run's says.

Every log line starts with the logger's own prefix (severity, wall-clock
time, thread id, source line), which no two processes share; the comparison
is of the bytes after that prefix, i.e. of everything the program itself
wrote."""
import os
import re
import subprocess

import pytest

from conftest import ML1M, PKG

pytestmark = pytest.mark.gpu

BIN = os.path.join(PKG, "bin")
TRAIN = os.path.join(ML1M, "train.csv")
VTR = os.path.join(ML1M, "validation_tr.csv")
VTE = os.path.join(ML1M, "validation_te.csv")

MODELS = {
    "ials": ["--model_name", "ials", "--dim", "8", "--uobs_weight", "0.1", "--l2_reg", "0.003"],
    "safer2": ["--model_name", "safer2", "--dim", "8", "--uobs_weight", "0.004", "--l2_reg",
               "0.004", "--bandwidth", "0.15", "--use_epanechnikov", "0", "--xi_iterations", "5",
               "--pd_iterations", "1", "--print_var_stats", "1", "--use_snr", "1"],
}


def _run_model(args, check=True):
    cmd = [os.path.join(BIN, "run_model"), "--train_data", TRAIN, "--test_train_data", VTR,
           "--test_test_data", VTE, "--seed", "1", "--print_train_stats", "0"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def _messages(log):
    """The log without each line's prefix and without the epoch timings."""
    out = []
    for line in log.split("\n"):
        m = re.match(r"^[IWEF]\d{4} \d\d:\d\d:\d\d\.\d{6} \d+ [\w.]+:\d+\] (.*)$", line)
        text = m.group(1) if m else line
        out.append(re.sub(r"Timer: Train=\d+", "Timer: Train=", text))
    return "\n".join(out)


def _after(msgs, marker, nth):
    """What follows the nth line that contains `marker`."""
    lines = msgs.split("\n")
    at = [i for i, l in enumerate(lines) if marker in l][nth - 1]
    return "\n".join(lines[at + 1:])


def _validation(log):
    msgs = _messages(log)
    return msgs[msgs.rindex("Validation Results"):]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_resumed_run_logs_the_uninterrupted_runs_validation(tmp_path, name):
    path = str(tmp_path / "model.frecsys")
    whole = _run_model(MODELS[name] + ["--epoch", "3"]).stderr
    first = _run_model(MODELS[name] + ["--epoch", "2", "--save_model", path]).stderr
    second = _run_model(MODELS[name] + ["--epoch", "1", "--load_model", path]).stderr
    assert re.findall(r"Epoch: (\d+), Timer", first) == ["0", "1"]
    assert re.findall(r"Epoch: (\d+), Timer", second) == ["2"]
    assert re.findall(r"Epoch: (\d+), Timer", whole) == ["0", "1", "2"]
    assert "Epoch 3:" in _validation(whole)
    assert _validation(second) == _validation(whole)
    assert "Initial Xi" not in second  # Initialize is skipped
    # and so does everything else the third epoch logged (xi, the weighted
    # loss, VaR): the resumed log after its three data-set lines is the whole
    # run's log after "Epoch: 1"
    assert _after(_messages(second), "num_tuples=", 3) == _after(_messages(whole), "Epoch: 1,", 1)


def test_wrong_training_data_is_refused(tmp_path):
    path = str(tmp_path / "model.frecsys")
    _run_model(MODELS["ials"] + ["--epoch", "1", "--save_model", path])
    cmd = [os.path.join(BIN, "run_model"), "--train_data", VTR, "--test_train_data", VTR,
           "--test_test_data", VTE, "--seed", "1"] + MODELS["ials"] + ["--epoch", "1",
                                                                      "--load_model", path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "tuples_checksum" in r.stderr
    r = _run_model(MODELS["safer2"] + ["--epoch", "1", "--load_model", path], check=False)
    assert r.returncode != 0 and "holds a ials model" in r.stderr
