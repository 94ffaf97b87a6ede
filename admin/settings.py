from admin.environment import env_settings


class Settings:
    """Run settings: `.env` holds admin/local.py's attributes; the launcher adds module_name, script_name,
    project_path, seed, name, severity, corruption_number (reference run_sampling.py:34-39,60-61) and, under --keyed_noise,
    keyed_noise; the document loop then keeps map_ref and map_dev here."""

    def __init__(self):
        self.set_default()

    def set_default(self):
        self.env = env_settings()
        self.use_gpu = True
