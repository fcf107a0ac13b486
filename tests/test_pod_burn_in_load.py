"""The pod builder and ``amd.com/gpu-burn-in-load-seconds``: on a GPU worker
template that also carries ``amd.com/gpu-burn-in: "true"`` it appends
``--load-seconds <n>`` to the startup probe's command and extends its timeout;
without the burn-in annotation, or with a value that is no number in (0, 60],
it changes nothing; and a template without it builds the pod it built before
the annotation existed (tests/golden/burn_in_pods.json, the pods of the commit
before)."""
import json
import logging
import os

import pytest

from kuberay_amd.common import pod as podlib
from kuberay_amd.models import RayCluster, RayNodeType
from kuberay_amd.testing import simple_raycluster
from kuberay_amd.utils import constants as C

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "burn_in_pods.json")
FQDN = "demo-head-svc.default.svc.cluster.local"
KEY = "amd.com/gpu-burn-in-load-seconds"


def _cluster(annotations, gpus=1):
    d = simple_raycluster("demo", gpus_per_worker=gpus).to_dict()
    tmpl = d["spec"]["workerGroupSpecs"][0]["template"]
    if annotations:
        tmpl.setdefault("metadata", {})["annotations"] = dict(annotations)
    return RayCluster.from_dict(d)


def _worker_pod(cluster):
    group = cluster.spec.worker_group_specs[0]
    template = podlib.default_worker_pod_template(cluster, group, "demo-worker-", FQDN, "6379")
    return podlib.build_pod(template, RayNodeType.WORKER, group.ray_start_params,
                            "6379", False, None, FQDN,
                            ray_version=cluster.spec.ray_version).to_dict()


def _startup(annotations, gpus=1):
    return _worker_pod(_cluster(annotations, gpus))["spec"]["containers"][0].get("startupProbe")


BURN_IN = {C.GPU_BURN_IN_ANNOTATION_KEY: "true"}


def test_annotation_key_and_limits():
    assert C.GPU_BURN_IN_LOAD_SECONDS_ANNOTATION_KEY == KEY
    assert C.GPU_BURN_IN_LOAD_MAX_SECONDS == 60
    assert C.GPU_BURN_IN_LOAD_PROBE_OVERHEAD_SECONDS >= 1


@pytest.mark.parametrize("value,flag,seconds", [("8", "8", 8), ("2.5", "2.5", 3),
                                                ("60", "60", 60), ("0.25", "0.25", 1),
                                                (" 4 ", "4", 4), ("1e1", "10", 10)])
def test_annotation_appends_the_flag_and_extends_the_timeout(value, flag, seconds):
    probe = _startup(dict(BURN_IN, **{KEY: value}))
    plain = _startup(BURN_IN)
    assert probe["exec"]["command"] == ["bash", "-c",
                                        f"{C.GPU_BURN_IN_PROBE_COMMAND} --load-seconds {flag}"]
    assert probe["timeoutSeconds"] == (C.GPU_BURN_IN_PROBE_TIMEOUT_SECONDS + seconds
                                       + C.GPU_BURN_IN_LOAD_PROBE_OVERHEAD_SECONDS)
    # nothing else of the probe, and nothing else of the pod, changes
    for d in (probe, plain):
        del d["exec"], d["timeoutSeconds"]
    assert probe == plain
    with_load = _worker_pod(_cluster(dict(BURN_IN, **{KEY: value})))
    without = _worker_pod(_cluster(BURN_IN))
    del with_load["metadata"]["annotations"][KEY]
    for d in (with_load, without):
        del d["spec"]["containers"][0]["startupProbe"]
    assert with_load == without


def test_probe_accepts_the_flag_the_builder_writes(monkeypatch):
    """The command the builder writes parses, and asks for that many seconds,
    also where the number is written with an exponent."""
    from kuberay_amd.gpu import probe as probe_cli
    command = _startup(dict(BURN_IN, **{KEY: "0.00005"}))["exec"]["command"][-1]
    prefix = "python -m kuberay_amd.gpu.probe "
    assert command.startswith(prefix)
    seen = {}

    def fake(**kwargs):
        seen.update(kwargs)
        raise probe_cli.GpuHealthError("stop here")
    monkeypatch.setattr(probe_cli, "check_gpu_burn_in", fake)
    assert probe_cli.main(command[len(prefix):].split()) == 2
    assert seen["load_seconds"] == pytest.approx(0.00005)


@pytest.mark.parametrize("other", [None, "false", "yes"])
def test_without_the_burn_in_annotation_it_does_nothing(other):
    annotations = {KEY: "8"}
    if other is not None:
        annotations[C.GPU_BURN_IN_ANNOTATION_KEY] = other
    assert _startup(annotations) is None
    pod = _worker_pod(_cluster(annotations))
    plain = _worker_pod(_cluster(None))
    pod["metadata"].pop("annotations")
    plain["metadata"].pop("annotations", None)
    assert pod == plain


def test_cpu_worker_gets_no_probe_either():
    assert _startup(dict(BURN_IN, **{KEY: "8"}), gpus=0) is None


@pytest.mark.parametrize("value", ["", "abc", "0", "-1", "60.5", "61", "nan", "inf", "-inf",
                                   "8s", "1,5", "true"])
def test_bad_values_are_ignored_and_logged(value, caplog):
    with caplog.at_level(logging.WARNING, logger="kuberay.pod"):
        probe = _startup(dict(BURN_IN, **{KEY: value}))
    assert probe == _startup(BURN_IN)
    assert probe["exec"]["command"][-1] == C.GPU_BURN_IN_PROBE_COMMAND
    assert probe["timeoutSeconds"] == C.GPU_BURN_IN_PROBE_TIMEOUT_SECONDS
    assert any(KEY in r.getMessage() and repr(value) in r.getMessage()
               for r in caplog.records)


def test_a_bad_value_is_warned_about_once(caplog):
    """Every reconcile builds the pod again: the repeats are debug lines."""
    annotations = dict(BURN_IN, **{KEY: "seven"})
    with caplog.at_level(logging.DEBUG, logger="kuberay.pod"):
        for _ in range(3):
            _startup(annotations)
    levels = [r.levelno for r in caplog.records if "'seven'" in r.getMessage()]
    assert levels == [logging.WARNING, logging.DEBUG, logging.DEBUG]


def test_good_values_are_not_logged(caplog):
    with caplog.at_level(logging.WARNING, logger="kuberay.pod"):
        _startup(dict(BURN_IN, **{KEY: "8"}))
        _startup(BURN_IN)
        _startup(None)
    assert not caplog.records


def test_pods_without_the_annotation_are_those_of_the_commit_before():
    """The golden file holds the worker pods the commit before this annotation
    built for the same three templates."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == ["burn_in", "cpu_worker", "plain"]
    assert _worker_pod(_cluster(None)) == golden["plain"]
    assert _worker_pod(_cluster(BURN_IN)) == golden["burn_in"]
    assert _worker_pod(_cluster(BURN_IN, gpus=0)) == golden["cpu_worker"]
