"""What derive_params() says without a device is what a context on the device answers: for five contexts without keys, every
getter against the report for the device's own CU count; and one run of a four-task DAG against dag_launch_choice()."""
import pytest

pytestmark = pytest.mark.gpu

CONTEXTS = [("TOY", "GINX", {}), ("STD128_OPT", "GINX", {}), ("STD128_OPT", "AP", {}), ("STD192_OPT", "AP", {}),
            ("STD128_OPT", "GINX", {"BCE_VARIANT": "1"})]


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("paramset,method,env", CONTEXTS, ids=["%s-%s%s" % (p, m, "".join("-%s=%s" % i for i in e.items())) for p, m, e in CONTEXTS])
def test_a_context_answers_what_derive_params_says(bce, cus, monkeypatch, paramset, method, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = bce.derive_params(getattr(bce, paramset), getattr(bce, method), cu_count=cus)
    assert d["status"] == bce.OK and d["cu_count"] == cus and d["variant"] == int(env.get("BCE_VARIANT", 0))
    cc = bce.BinFHEContext(getattr(bce, paramset), getattr(bce, method))
    try:
        want = {"n": d["n"], "N": d["N"], "q": d["q"], "Q": d["Q64"], "qKS": d["qKS"], "baseKS": d["baseKS"], "dKS": d["dKS"],
                "baseG": 1 << d["gBits"], "dG": d["dG"], "baseR": d["baseR"], "dR": d["dR"], "method": getattr(bce, method), "psi": d["psi"]}
        assert cc.params == want
        assert (cc.is64(), cc.fp64()) == (bool(d["is64"]), bool(d["fp64"]))
        assert (cc.forward_units(), cc.forward_mfma(), cc.lazy_arithmetic()) == (d["fwd_units"], d["fwd_mfma"], d["lazy"])
        assert cc.forward_transforms_per_step() == d["forward_transforms"]
        assert tuple(cc.launch_capacity()) == (d["capacity_lone"], d["capacity_full"])
        assert cc.bytes_per_bootstrap_parts() == {"bsk": d["bytes_bsk"], "ksk": d["bytes_ksk"], "ct": d["bytes_ct"]}
        assert bool(cc.dag_supported()) == bool(d["dag"])
    finally:
        cc.close()


def test_a_dag_run_uses_what_dag_launch_choice_says(bce, cus):
    d = bce.derive_params(bce.STD128_OPT, bce.GINX, cu_count=cus)
    cc = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    try:
        cc.KeyGen(7)
        tasks = [(bce.AND, 0, 1, 2), (bce.OR, 0, 1, 3), (bce.NAND, 2, 3, 4), (bce.NOR, 2, 4, 5)]    # depth 3
        cc.pool_reserve(6)
        cc.Encrypt([1, 0], [0, 1])
        dag = cc.dag_create(tasks)
        for wg in (0, 1, 2):
            choice = bce.dag_launch_choice(d, depth=3, items=len(tasks), workgroups_per_cu=wg)
            assert choice["wps"] == (4 if wg == 2 else 2) and choice["grid"] == cus * choice["wps"] // 2
            cc.dag_set_limits(workgroups_per_cu=wg)
            cc.dag_run(dag)
            cc.synchronize()
            last = cc.dag_last_run()
            assert (last["done"], last["abort"], last["workgroups_per_cu"]) == (len(tasks), 0, choice["wps"] // 2)
        assert list(cc.Decrypt([2, 3, 4, 5])) == [0, 1, 1, 0]
        cc.dag_destroy(dag)
    finally:
        cc.dag_set_limits()
        cc.close()
