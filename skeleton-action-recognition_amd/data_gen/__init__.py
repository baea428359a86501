"""The reference's data_gen package, as far as it is needed at run time: `preprocess.pre_normalization` on the device.  (Bone and
motion are computed inside the data_bn kernels, sar_amd/bone.py; TFRecord shards are read by sar_amd/tfrecord.py.)"""
from .preprocess import pre_normalization  # noqa: F401
