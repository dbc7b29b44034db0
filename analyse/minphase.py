"""Shim: re-exports audio_analysis_amd.analyse.minphase; `python -m analyse.minphase ...` runs its command line."""
import sys as _sys

import audio_analysis_amd.analyse.minphase as _impl

if __name__ == "__main__":
    _impl.main()
else:
    _sys.modules[__name__] = _impl
