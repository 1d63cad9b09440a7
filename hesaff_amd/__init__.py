"""hesaff_amd -- MI355X-native Hessian-Affine + SIFT (drop-in for perdoch/hesaff's detect+describe path).

Python host mirror over the C ABI (include/hesaff_amd.h -> hesaff_amd/libhesaff_amd.so).
The library is HIP only: there is no CPU fallback, creating a context without a gfx950
device raises HesaffError.

Input: 8-bit images (HesaffContext.detect_batch and its kin) or float32 grey planes, the reference's own
CV_32FC1 detector input (the *_f32 methods: detect_batch_f32, detect_regions_f32, detect_batch_cb_f32,
pyramid_f32 on numpy arrays, detect_batch_device_f32 on a torch tensor in device memory).

Detect, choose, describe the chosen: HesaffContext.detect_regions returns every Hessian keypoint as a record, and
HesaffContext.describe_regions (describe_regions_f32) runs the rest of the chain on the records the caller hands back,
or on keypoints of the caller's own, entering at findAffineShape (FROM_POINTS) or at the affine shape (FROM_SHAPES).
"""
from ._binding import (  # noqa: F401
    HesaffError,
    HesaffContext,
    Params,
    KEYPOINT_DTYPE,
    REGION_DTYPE,
    Region,
    FROM_POINTS,
    FROM_SHAPES,
    ORI_UP,
    ORI_DOMINANT,
    DESC_SIFT,
    DESC_ROOTSIFT,
    default_params,
    format_sift,
    format_sift_mt,
    write_sift,
    write_sift_batch,
    write_bin,
    read_bin,
    BIN_ROW_DTYPE,
    OUT_TEXT,
    OUT_BIN,
    OUT_WORDS,
    WORDS_ROW_DTYPE,
    read_vocabulary,
    write_vocabulary,
    read_vocabulary_cells,
    write_vocabulary_cells,
    read_words,
    write_words,
    expand_rows,
    EMBED_BITS,
    embedding_projection,
    read_embedding,
    write_embedding,
    read_signatures,
    write_signatures,
    read_index_file,
    write_index_file,
    read_image,
    read_pnm,
    read_jpeg_coefficients,
    JpegLayout,
    ellipse,
    lib_path,
    load_library,
    host_plan,
    table_gauss_mask,
    table_circ_gauss_mask,
    table_sift_bins,
    table_gauss_kernel,
)
