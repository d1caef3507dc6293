"""No environment variable picks a kernel path: the only ones the Python package reads say where
the libraries and the compiler are. Paths are decided in vrvq_amd/paths.py; the three test
switches (ops.X3, model.RVQ_PROJ, discriminator.MPD_1D) are plain attributes, True by default."""
import glob
import os
import re

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vrvq_amd")
ALLOWED = {"VRVQ_LIB", "VRVQ_TORCH_LIB", "VRVQ_OFFLOAD_ARCH", "HIPCC"}
READ = re.compile(r"""os\.environ\.get\(\s*["'](\w+)["']|os\.environ\[\s*["'](\w+)["']\s*\]|"""
                  r"""os\.getenv\(\s*["'](\w+)["']""")


def test_only_library_and_toolchain_locations_are_read():
    files = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert len(files) >= 15
    names = set()
    for path in files:
        with open(path) as f:
            src = f.read()
        reads = [m for m in READ.finditer(src)]
        # every mention of the environment is a read of a literal name this test can see
        assert len(re.findall(r"\benviron\b|\bgetenv\b|\bputenv\b", src)) == len(reads), path
        names |= {next(g for g in m.groups() if g) for m in reads}
    assert names == ALLOWED


def test_switches_are_plain_attributes_on_by_default():
    from vrvq_amd import discriminator, model, ops
    assert ops.X3 is True and model.RVQ_PROJ is True and discriminator.MPD_1D is True
    for mod, gone in ((ops, ("RU256_SPLIT", "X3_STRIDED", "RU_FUSED_CHANNELS")),
                      (discriminator, ("MPD_GEMM",))):
        for name in gone:
            assert not hasattr(mod, name), name
    from vrvq_amd import layers, train
    assert not hasattr(train, "TRAIN_X3") and "fused" not in vars(layers.ResidualUnit)
