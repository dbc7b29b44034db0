"""Shim: re-exports audio_analysis_amd.analyse.edr; `python -m analyse.edr ...` runs its command line."""
import sys as _sys

import audio_analysis_amd.analyse.edr as _impl

if __name__ == "__main__":
    _impl.main()
else:
    _sys.modules[__name__] = _impl
