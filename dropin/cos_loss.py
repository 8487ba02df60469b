"""Drop-in shim: `import cos_loss` (the reference's /root/reference/cos_loss.py) resolves to the MI355X-native module."""
from tinyrecurrentunet_amd.cos_loss import *  # noqa: F401,F403
from tinyrecurrentunet_amd import cos_loss as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("__")]
globals().update({n: getattr(_impl, n) for n in dir(_impl) if not n.startswith("__")})
