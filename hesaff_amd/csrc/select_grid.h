// select_grid.h -- the integer arithmetic of the keypoint selection's pixel and grid-cell rules (kernels_select.h), HIP-free so that
// a stand-alone host program can check it (tests/native/grid_cell_check.cpp): host and device run these lines.
#pragma once

#if defined(__HIPCC__)
#define HS_SG_HD __host__ __device__ __forceinline__
#else
#define HS_SG_HD inline
#endif

#define HS_GRID_MAX_CELLS 64   // hesaff_set_keypoint_grid: rows * cols <= 64

// The pixel of a keypoint coordinate v along an axis of `size` pixels: clamp((int)(v + 0.5f), 0, size - 1), the add in binary32, the
// conversion truncating (the masks' rule and the grid's).
HS_SG_HD int hs_sel_pixel(float v, int size)
{
   const int p = (int)(v + 0.5f);
   return p < 0 ? 0 : (p > size - 1 ? size - 1 : p);
}

// The grid cell, of n along an axis of `size` pixels, that holds pixel pos (0 <= pos < size, 1 <= n): the c with
// c * size / n <= pos < (c + 1) * size / n in integer division - the cell ranges of OpenCV's GridAdaptedFeatureDetector - in closed
// form.  NOT pos * n / size, which differs wherever size is no multiple of n.  (pos + 1) * n stays inside int32 for every image
// the library takes (size <= 65535) and n <= 64.
HS_SG_HD int hs_grid_cell_1d(int pos, int n, int size) { return ((pos + 1) * n - 1) / size; }

// cell index of pixel (row, col) of a W x H image under an R x C grid: rows of cells outermost
HS_SG_HD int hs_grid_cell(int row, int col, int R, int C, int W, int H) { return hs_grid_cell_1d(row, R, H) * C + hs_grid_cell_1d(col, C, W); }
