"""The fork's resnet18.py is model_v1's: the same parameter containers."""
try:                                    # `from model import resnet18` (fork layout, htr-vt_amd/sgm_mms on sys.path)
    from htrvt_amd.model.resnet18 import BasicBlock, ResNet18  # noqa: F401
except ImportError:
    from ...model.resnet18 import BasicBlock, ResNet18  # noqa: F401
