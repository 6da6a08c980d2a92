// P/Invoke surface of libsnappier_hip_frame_append.so -- one declaration per function of include/snappier_hip_frame_append.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameAppend
{
    private const string Lib = "snappier_hip_frame_append";                     // libsnappier_hip_frame_append.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): bytes appended in place to framed streams kept with their index
    // (the five dIdx* pointers are the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes, the five dNew* the index after the call; dOutBound may be IntPtr.Zero)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_append_indexed_workspace(uint nstreams, uint maxTails, uint maxSlots, uint chunkBytes);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_append_indexed_batch(IntPtr ctx, IntPtr dBuf, IntPtr dBufOff, IntPtr dBufLen, IntPtr dBufCap, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dSrc, IntPtr dSrcOff, IntPtr dSrcLen, uint chunkBytes, uint maxTails, uint maxSlots, IntPtr dNewLen, IntPtr dStatus, IntPtr dNewFirst, IntPtr dNewStart, IntPtr dNewPos, IntPtr dNewTotal, IntPtr dNewTail, IntPtr dOutBound, IntPtr dWork, IntPtr dResult);
}
