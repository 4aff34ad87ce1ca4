"""n3dt: MI355X-native volumetric head rendering behind NeRF-3DTalker's HeadNeRFNet interface."""
from .options import BaseOptions  # noqa: F401
from .headnerf import HeadNeRFNet, NeuralRenderer, MLPforNeRF  # noqa: F401
from .audio import Audio2style  # noqa: F401
from .mel import MelFrontend, MelStream, mel_basis  # noqa: F401
from .optim import FlatAdam  # noqa: F401
from .eval_utils import image_metrics, calc_eval_metrics, LPIPS, SyncNet, SyncMeter  # noqa: F401
from .wav2lip import Wav2Lip, Wav2LipClip, load_wav2lip  # noqa: F401
from .s3fd import S3FD, load_s3fd  # noqa: F401
from .face_recon import FaceRecon, load_face_recon  # noqa: F401
from .fan import FAN, load_fan  # noqa: F401
from .head_mask import HeadMask, load_head_mask  # noqa: F401
from .train import validate  # noqa: F401
from . import checkpoint, render_utils, parallel, train, fitting, audio, optim, eval_utils, mel, syncnet, wav2lip, s3fd, face_recon, fan, head_mask  # noqa: F401,E402
