"""Drop-in for /root/reference/lib/ops/__init__.py (which re-exports mmcv.ops).

RoIAlign / roi_align are on the CIM training path of every shipped config (model_builder.py:229-231); RoIPool / roi_pool
serve ROI_XFORM_METHOD=RoIPoolF (model_builder.py:227-228; ops/roi_pool.py).  nms / soft_nms - eval-only box
ops whose work cim_amd.detect does - are kept importable and raise if called - SURVEY.md section 2.2."""
from .bn_act import bn_act
from .bn_train import bn_act_train
from .conv1x1 import conv1x1_bn_act
from .conv3x3 import conv3x3_bias_act, conv3x3_bn_act, conv7x7_bn_act, conv7x7_bn_act_train
from .pool import max_pool2d, upsample_nearest
from .roi_align import RoIAlign, roi_align, roi_align_maskcat
from .roi_pool import RoIPool, roi_pool, roi_pool_maskcat


def _out_of_scope(name):
    def fn(*args, **kwargs):
        raise NotImplementedError("%s is not on the CIM training hot path and is not provided by cim_amd" % name)
    fn.__name__ = name
    return fn


nms = _out_of_scope("nms")
soft_nms = _out_of_scope("soft_nms")

__all__ = ["RoIPool", "RoIAlign", "roi_pool", "roi_align", "nms", "soft_nms", "roi_align_maskcat", "roi_pool_maskcat", "bn_act", "bn_act_train", "conv1x1_bn_act", "conv3x3_bn_act", "conv3x3_bias_act", "conv7x7_bn_act", "conv7x7_bn_act_train", "max_pool2d", "upsample_nearest"]
