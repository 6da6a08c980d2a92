// P/Invoke surface of libsnappier_hip_frame_update.so -- one declaration per function of include/snappier_hip_frame_update.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameUpdate
{
    private const string Lib = "snappier_hip_frame_update";                     // libsnappier_hip_frame_update.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): requests that replace decoded bytes of framed streams through their index
    // (the five dIdx* pointers are the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes; dNewPos and dOutBound may be IntPtr.Zero)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_write_indexed_workspace(uint nstreams, uint nreq, uint maxSlots, ulong stageCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_write_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dSrc, IntPtr dReqStream, IntPtr dReqOff, IntPtr dReqLen, IntPtr dSrcOff, uint nreq, uint maxSlots, ulong stageCap, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dReqStatus, IntPtr dNewPos, IntPtr dOutBound, IntPtr dWork, IntPtr dResult);
}
