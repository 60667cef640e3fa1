"""Import-name shim: `from simple_knn._C import distCUDA2` (gaustar_scene/sugar_model.py:9,
gaussian_splatting/scene/gaussian_model.py:20) resolves to the MI355X-native search of gaustar_amd.knn when this
repository's root is on sys.path, so the reference's callers import and run unchanged."""
