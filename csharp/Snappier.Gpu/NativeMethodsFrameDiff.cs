// P/Invoke surface of libsnappier_hip_frame_diff.so -- one declaration per function of include/snappier_hip_frame_diff.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameDiff
{
    private const string Lib = "snappier_hip_frame_diff";                       // libsnappier_hip_frame_diff.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    internal const uint SNP_DIFF_PREFIX = 1, SNP_DIFF_SUFFIX = 2, SNP_DIFF_EXACT = 4;

    // ---- batch, device pointers (asynchronous on the context's stream): longest common prefix and suffix of pairs of windows of what framed streams kept with their index decode to
    // (per side the streams and the five dIdx* arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes; per side three dReq* arrays -- dReqStream holds uint;
    //  dLenA, dLenB, dPrefix, dSuffix hold ulong, dStatus int)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_diff_indexed_workspace(uint nreq, ulong maxRows, ulong scratchCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_diff_indexed_batch(IntPtr ctx, IntPtr dInA, IntPtr dInOffA, IntPtr dInLenA, uint nstreamsA, IntPtr dIdxFirstA, IntPtr dIdxStartA, IntPtr dIdxPosA, IntPtr dIdxTotalA, IntPtr dIdxTailA, ulong nentriesA, IntPtr dInB, IntPtr dInOffB, IntPtr dInLenB, uint nstreamsB, IntPtr dIdxFirstB, IntPtr dIdxStartB, IntPtr dIdxPosB, IntPtr dIdxTotalB, IntPtr dIdxTailB, ulong nentriesB, IntPtr dReqStreamA, IntPtr dReqOffA, IntPtr dReqLenA, IntPtr dReqStreamB, IntPtr dReqOffB, IntPtr dReqLenB, uint nreq, uint flags, ulong maxRows, ulong scratchCap, IntPtr dLenA, IntPtr dLenB, IntPtr dPrefix, IntPtr dSuffix, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
