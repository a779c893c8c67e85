from .opt import (
    PathType,
    dyn_structure,
    get_config_class_snake_case_name,
    get_generic_classes,
    is_path_type,
    normalize_to_probs,
    read_json_file,
    rng_choice,
    rng_choice_with_size,
    rng_shuffle,
    sample_cv_resize_interpolation,
)
