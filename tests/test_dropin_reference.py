"""b-1: `install_as_lib()` / `uninstall_as_lib()` put cim_amd in the reference's module namespace and take it out again."""
import sys


def test_install_uninstall_roundtrip():
    import cim_amd
    from cim_amd.core import config as own
    cim_amd.install_as_lib()
    try:
        import ops                                  # noqa: F401  resolves without the reference tree
        assert sys.modules["ops"].__name__ == "cim_amd.ops"
        import modeling.heads as h                  # noqa: F401  parent package `modeling` may not exist: alias only
    except ModuleNotFoundError:
        pass                                        # without lib/ on sys.path the parent package is absent - fine
    finally:
        cim_amd.uninstall_as_lib()
    assert "ops" not in sys.modules
    assert own.cfg.target() is own._own
