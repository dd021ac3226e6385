from audiolab_amd.wrappers.compare import Compare  # noqa: F401
